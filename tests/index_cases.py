"""Crafted keys for the contig index (csrc/index_common.h, map_kernels.h index_*): chosen home slots and tag bytes, so that a small
table holds what random keys never give it -- probe sequences longer than the eight tags of one load, sequences across the end of the
table, refuted tag matches, the key that equals the empty marker, heavily duplicated keys.  Every case is a set of arrays for
sketch_from_arrays -> index -> map, with what the oracle's index (another hash, a state field, no sentinel key) makes of them.

home(), tag() and table_bits() restate the kernels; tests/test_index_edges.py::test_source_literals holds them to the sources."""
import functools

import numpy as np

import oracle
from helpers import contig_ids

M64 = (1 << 64) - 1
MULT = 0x9E3779B97F4A7C15           # index_home: (key * MULT) >> (64 - bits)
INV = pow(MULT, -1, 1 << 64)        # MULT is odd
ALL_ONES = M64                      # NTL_INF, the empty marker: kept beside the table (IndexSpecial)
K = 24
CTG_LEN = 5000
PER_CTG = 150                       # records per contig, about


def home(key, bits):
    return ((key * MULT) & M64) >> (64 - bits)


def tag(key):
    return ((key >> 20) & 0xFE) | 1


index_tag = tag  # (keys_at has a parameter of that name)


def table_bits(count):
    """the table of `count` contig minimizer records (the all-ones key among them) has 2^bits slots"""
    bits = 10
    while (1 << bits) < 2 * count + 2:
        bits += 1
    return bits


def keys_at(slot, bits, n, rng, tag=None, avoid=()):
    """n distinct keys, none all-ones and none in `avoid`, whose home slot in a table of 2^bits slots is `slot`, with the tag byte
    `tag` if one is given: (slot << (64 - bits) | low) * MULT^-1 has that home for every low; low is drawn until the tag fits."""
    assert 0 <= slot < (1 << bits) and (tag is None or (tag & 1 and 0 < tag < 256))
    out, seen = [], set(avoid)
    while len(out) < n:
        for low in rng.integers(0, 1 << (64 - bits), 256):
            key = (((slot << (64 - bits)) | int(low)) * INV) & M64
            if key == ALL_ONES or key in seen or (tag is not None and index_tag(key) != tag):
                continue
            assert home(key, bits) == slot
            out.append(key); seen.add(key)
            if len(out) == n:
                break
    return out


def keys_between(lo, hi, bits, n, rng, avoid=()):
    """n distinct keys with random homes in [lo, hi)"""
    out = []
    for s in rng.integers(lo, hi, n):
        out += keys_at(int(s), bits, 1, rng, avoid=set(avoid) | set(out))
    return out


def random_keys(n, bits, rng, keep_out=()):
    """n distinct random keys whose homes lie in none of the (lo, hi) slot ranges of keep_out"""
    out = set()
    while len(out) < n:
        key = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        if key != ALL_ONES and key != 0 and not any(lo <= home(key, bits) < hi for lo, hi in keep_out):
            out.add(key)
    return sorted(out, key=lambda _k: rng.random())


def occupied(keys, bits):
    """the slots that a table of these distinct keys occupies (linear probing: the same set whatever the order of the inserts)"""
    mask, occ = (1 << bits) - 1, set()
    for key in keys:
        s = home(key, bits)
        while s in occ:
            s = (s + 1) & mask
        occ.add(s)
    return occ


def first_empty(occ, slot, bits):
    while slot in occ:
        slot = (slot + 1) & ((1 << bits) - 1)
    return slot


def span(slot, n, bits):
    return {(slot + i) & ((1 << bits) - 1) for i in range(n)}


class Case:
    """present: keys inserted once; copies: {key: (times, "same" | "across" | "any")} -- all in one contig, in different contigs, wherever;
    absent: keys only the reads ask for.  n_ctg contigs of CTG_LEN, the records on the contigs `on` (all of them by default), the keys
    dealt to the contigs in a seeded random order, positions increasing within a contig, strands random.  One read per contig with
    records: the contig's keys in contig order (a key it holds twice, once), the contig's strands, positions 40 apart, the absent keys at
    random places of random reads -- every key the lookup finds then survives the map's filters and is a hit record."""

    def __init__(self, name, rng, bits, present, absent, copies=None, n_ctg=None, on=None):
        self.name, self.bits = name, bits
        copies = copies or {}
        assert len(set(present)) == len(present) and not set(present) & set(copies) and not set(absent) & (set(present) | set(copies))
        nrec = len(present) + sum(t for t, _ in copies.values())
        if n_ctg is None:
            n_ctg = max(3, -(-nrec // PER_CTG))
        on = list(range(n_ctg)) if on is None else list(on)
        per = {c: [] for c in on}
        for key in present:
            per[on[int(rng.integers(0, len(on)))]].append(key)
        for key, (times, how) in copies.items():
            first = int(rng.integers(0, len(on)))
            for i in range(times):
                c = first if how == "same" else (first + i) % len(on) if how == "across" and i < len(on) else int(rng.integers(0, len(on)))
                per[on[c]].append(key)
        counts = np.zeros(n_ctg, np.uint64)
        ch, cp, cs = [], [], []
        reads = []
        for c in on:
            keys = per[c]
            order = rng.permutation(len(keys))
            keys = [keys[i] for i in order]
            assert len(keys) <= (CTG_LEN - K) // 2
            pos = np.sort(rng.choice(CTG_LEN - K, len(keys), replace=False))
            strands = rng.integers(0, 2, len(keys))
            counts[c] = len(keys)
            ch += keys; cp += [int(p) for p in pos]; cs += [int(s) for s in strands]
            toks, seen = [], set()
            for key, s in zip(keys, strands):
                if key not in seen:
                    seen.add(key)
                    toks.append((key, int(s)))
            if toks:
                reads.append(toks)
        if not reads:
            reads = [[], []]
        for key in absent:
            toks = reads[int(rng.integers(0, len(reads)))]
            toks.insert(int(rng.integers(0, len(toks) + 1)), (key, int(rng.integers(0, 2))))
        self.n_records = len(ch)
        assert self.n_records == nrec and table_bits(nrec) == bits, (name, nrec, table_bits(nrec), bits)
        self.coff = np.zeros(n_ctg + 1, np.uint64)
        np.cumsum(counts, out=self.coff[1:])
        self.ch, self.cp, self.cs = np.array(ch, np.uint64), np.array(cp, np.uint32), np.array(cs, np.uint8)
        self.ctg_len = np.full(n_ctg, CTG_LEN, np.uint32)
        self.unique = set(present) | {key for key, (t, _) in copies.items() if t == 1}
        self.stored = set(present) | set(copies)
        self.reads = self._read_arrays(reads)
        self.all_hit = self._read_arrays([[t for t in toks if t[0] in self.unique] for toks in reads])
        self._exp = None

    @staticmethod
    def _read_arrays(reads):
        roff = np.zeros(len(reads) + 1, np.uint64)
        np.cumsum([len(t) for t in reads], out=roff[1:])
        rh = np.array([key for t in reads for key, _ in t], np.uint64)
        rp = np.array([40 * i for t in reads for i in range(len(t))], np.uint32)
        rs = np.array([s for t in reads for _, s in t], np.uint8)
        rlen = np.array([max(CTG_LEN, 40 * len(t) + K) for t in reads], np.uint32)
        return roff, rlen, rh, rp, rs

    def table_keys(self):
        """the keys that take a slot (every stored key but the all-ones one; a dropped key keeps its slot)"""
        return [key for key in self.stored if key != ALL_ONES]

    def expected(self):
        """(the oracle's records of the reads, its index size, the read minimizers its index holds), made once; the inputs are built so
        that the oracle alone meets the conditions every case asserts of the product"""
        if self._exp is None:
            oix = oracle.Index(self.ch, contig_ids(self.coff) if len(self.ch) else np.empty(0, np.uint32), self.cp, self.cs)
            roff, rlen, rh, rp, rs = self.reads
            exp = oracle.map_reads(oix, self.ctg_len, roff, rlen, rh, rp, rs, k=K, threads=0)
            found = sum(1 for key in rh if oix.lookup(int(key)) is not None)
            assert len(oix) == len(self.unique), self.name
            assert found == sum(1 for key in rh if int(key) in self.unique) == len(exp["hits"]), self.name
            assert found == len(self.all_hit[2]), self.name
            if self.stored:
                assert 0 < found < len(rh), self.name
            self._exp = (exp, len(oix), found)
        return self._exp


# ---------------------------------------------------------------- the cases

T_SHARED = 0x5B  # the one tag several keys of a cluster share


def _cluster(slot, bits, n, rng, shared=None):
    """n keys of one home; the first `shared` of them (a third by default, two at the least) with the tag T_SHARED, no other with it"""
    shared = max(2, n // 3) if shared is None else shared
    keys = keys_at(slot, bits, shared, rng, tag=T_SHARED)
    while len(keys) < n:
        keys += [key for key in keys_at(slot, bits, 1, rng, avoid=keys) if tag(key) != T_SHARED]
    return keys


def _cluster_absent(slot, bits, cluster, rng):
    """absent keys of the cluster's home: three with a tag no cluster key has, three with the tag several cluster keys share"""
    used = {tag(key) for key in cluster}
    fresh = next(t for t in range(0x21, 256, 2) if t not in used)
    return keys_at(slot, bits, 3, rng, tag=fresh, avoid=cluster) + keys_at(slot, bits, 3, rng, tag=T_SHARED, avoid=cluster)


def _one_home(name, seed, n, slot, bits=10, also_absent_at=()):
    """one cluster of n keys at `slot` (cases a, b), forty keys far from it, absent keys of the same home and of the homes given"""
    rng = np.random.default_rng(seed)
    nslots = 1 << bits
    cluster = _cluster(slot, bits, n, rng)
    far = keys_between(nslots // 4 + 64, nslots // 4 + 320, bits, 40, rng) if slot < nslots // 4 or slot > nslots // 2 else \
        keys_between(nslots // 2 + 64, nslots // 2 + 320, bits, 40, rng)
    absent = _cluster_absent(slot, bits, cluster, rng)
    for s in also_absent_at:
        absent += keys_at(s & (nslots - 1), bits, 2, rng, avoid=cluster + absent)
        absent += keys_at(s & (nslots - 1), bits, 1, rng, tag=T_SHARED, avoid=cluster + absent)
    absent += random_keys(5, bits, rng)
    case = Case(name, rng, bits, cluster + far, absent)
    occ = occupied(case.table_keys(), bits)
    assert span(slot, n, bits) <= occ and (slot + n) & (nslots - 1) not in occ, name  # depths 0 .. n - 1, then an empty slot
    case.occ = occ
    return case


def case_a(n):
    """a. one home, growing clusters: 7 and 8 end inside the eight tags, 9 and more go on slot by slot"""
    return _one_home(f"a-{n}", 100 + n, n, 300, also_absent_at=(300 + n // 2, 300 + n - 1))


# (keys, home): every home of 1016 .. 1023; (8, 1016) ends on slot 1023 and (15, 1016) on slot 6
B_CLUSTERS = [(7, 1020), (8, 1016), (9, 1023), (10, 1021), (15, 1016), (16, 1018), (40, 1019), (9, 1017), (12, 1022)]


def case_b(n, slot, bits=10):
    """b. wrap: the same clusters at the end of the table, spilling into slots 0 ...; absent keys of every home 1016 .. 1023 and of the
    slots behind the seam"""
    nslots = 1 << bits
    case = _one_home(f"b-{n}-at-{slot}", 200 + 41 * n + slot, n, slot, bits, also_absent_at=list(range(nslots - 8, nslots + 8)))
    if (n, slot) == (8, nslots - 8):  # an absent lookup (one of every home 1016 .. 1023) whose first empty slot is exactly slot 0
        assert all(first_empty(case.occ, s, bits) == 0 for s in range(nslots - 8, nslots))
    if (n, slot) == (15, nslots - 8):  # ... exactly slot 7: from home 1023 the eight tags are all taken and the walk goes on at slot 7
        assert all(first_empty(case.occ, s, bits) == 7 for s in list(range(nslots - 8, nslots)) + list(range(7)))
    return case


def case_b_seam():
    """twelve keys whose homes are the consecutive slots 1019 .. 1023: matches and empty slots on both sides of the seam"""
    rng = np.random.default_rng(77)
    bits = 10
    keys, absent = [], []
    for slot, n in zip(range(1019, 1024), (3, 2, 2, 2, 3)):
        keys += keys_at(slot, bits, 1, rng, tag=T_SHARED, avoid=keys) + keys_at(slot, bits, n - 1, rng, avoid=keys)
    for slot in list(range(1017, 1024)) + list(range(0, 9)):
        absent += keys_at(slot, bits, 1, rng, tag=T_SHARED, avoid=keys + absent) + keys_at(slot, bits, 1, rng, avoid=keys + absent)
    case = Case("b-seam12", rng, bits, keys + keys_between(300, 600, bits, 40, rng), absent + random_keys(5, bits, rng))
    occ = occupied(case.table_keys(), bits)
    assert span(1019, 12, bits) <= occ and not {1017, 1018, 7, 8} & occ
    assert sum(1 for key in keys if home(key, bits) == 1023) == 3
    return case


def case_c():
    """c. extreme tags: clusters of 3 .. 8 keys that all carry the tag 0x01, the same with 0xFF, each followed by an empty slot; three
    more, alternating, one empty slot apart, so that one load of eight tags sees 0x01 and 0xFF on both sides of an empty byte"""
    rng = np.random.default_rng(303)
    bits = 10
    keys, absent, clusters = [], [], []
    layout = [(40 + 60 * i, 3 + i % 6, (0x01, 0xFF)[i // 6]) for i in range(12)] + [(800, 3, 0x01), (804, 3, 0xFF), (808, 3, 0x01)]
    for slot, n, t in layout:
        cl = keys_at(slot, bits, n, rng, tag=t, avoid=keys)
        keys += cl
        clusters.append((slot, n))
        absent += keys_at(slot, bits, 2, rng, tag=t, avoid=keys + absent)           # the same home, the same tag
        absent += keys_at(slot, bits, 2, rng, tag=t ^ 0xFE, avoid=keys + absent)    # the same home, the other extreme tag
    case = Case("c-extreme-tags", rng, bits, keys, absent + random_keys(5, bits, rng))
    occ = occupied(case.table_keys(), bits)
    for slot, n in clusters:
        assert span(slot, n, bits) <= occ and slot + n not in occ and slot - 1 not in occ
    return case


D_VARIANTS = ["absent", "once", "twice-in-one-contig", "three-times-across-contigs", "alone"]


def case_d(variant):
    """d. the all-ones key (absent, once, twice in one contig, three times across contigs, the only key of the index) and the key 0
    (present with the all-ones key once or twice, absent otherwise); the reads always ask for both"""
    rng = np.random.default_rng(400 + D_VARIANTS.index(variant))
    bits = 10
    if variant == "alone":
        return Case("d-alone", rng, bits, [ALL_ONES], [0] + random_keys(6, bits, rng))
    keys = _cluster(500, bits, 9, rng) + keys_between(100, 400, bits, 40, rng)
    absent = _cluster_absent(500, bits, keys[:9], rng) + random_keys(5, bits, rng)
    copies = {}
    if variant == "absent":
        absent += [ALL_ONES, 0]
    elif variant == "once":
        keys += [ALL_ONES, 0]
    elif variant == "twice-in-one-contig":
        copies[ALL_ONES] = (2, "same")
        keys += [0]
    else:
        copies[ALL_ONES] = (3, "across")
        absent += [0]
    case = Case("d-" + variant, rng, bits, keys, absent, copies)
    assert (ALL_ONES in case.unique) == (variant == "once")
    assert ALL_ONES in case.reads[2] and 0 in case.reads[2]
    return case


def case_e(bits=10):
    """e. duplicates inside a twelve-key cluster of one home: keys inserted 2, 3 and 200 times (and two more twice: five dropped keys
    in twelve slots, so whatever the order of the inserts one of them lies among the first eight slots and one behind them), in one
    contig and across contigs, the 200 copies all over the record array.  The cluster's slots all have bit 4 of the slot number set
    (the duplicate bitmap's word is indexed with slot & 31).  bits = 12: the same among 1500 records, eight workgroups of inserts."""
    rng = np.random.default_rng(500 + bits)
    nslots = 1 << bits
    slot = nslots // 2 + 16
    cluster = _cluster(slot, bits, 12, rng)
    assert all((s & 31) >= 16 for s in span(slot, 12, bits))
    dropped = [cluster[0], cluster[3], cluster[5], cluster[8], cluster[10]]  # cluster[0] shares its tag with three kept keys
    copies = dict(zip(dropped, [(2, "same"), (3, "across"), (200, "any"), (2, "across"), (2, "same")]))
    kept = [key for key in cluster if key not in copies]
    filler = random_keys(250 if bits == 10 else 1284, bits, rng, keep_out=[(slot - 40, slot + 40)])
    case = Case(f"e-dup-{nslots}", rng, bits, kept + filler, _cluster_absent(slot, bits, cluster, rng) + random_keys(5, bits, rng), copies)
    assert span(slot, 12, bits) <= occupied(case.table_keys(), bits)
    assert not set(dropped) & case.unique and set(dropped) <= set(int(h) for h in case.reads[2])  # the dropped keys are asked for
    n_ctg = len(case.ctg_len)
    big = contig_ids(case.coff)[case.ch == np.uint64(dropped[2])]
    assert len(big) == 200 and len(set(big.tolist())) == n_ctg and max(np.bincount(big)) > 1  # in one contig and across contigs
    return case


F_SIZES = [(511, 10), (512, 11), (1023, 11), (1024, 12)]


def case_f(nrec, bits):
    """f. sizes: 511 records fit the 1024 table exactly, 512 take 2048, 1023 take 2048, 1024 take 4096 -- each with a cluster of 10 of
    one home across the end of ITS table and one of 10 in its middle, among random keys"""
    assert table_bits(nrec) == bits and table_bits(nrec - 1) == bits - (nrec in (512, 1024))
    rng = np.random.default_rng(600 + nrec)
    nslots = 1 << bits
    wrap, mid = _cluster(nslots - 4, bits, 10, rng), _cluster(nslots // 2, bits, 10, rng)
    out = [(nslots - 64, nslots), (0, 32), (nslots // 2 - 40, nslots // 2 + 40)]
    absent = _cluster_absent(nslots - 4, bits, wrap, rng) + _cluster_absent(nslots // 2, bits, mid, rng) + random_keys(20, bits, rng)
    case = Case(f"f-{nrec}", rng, bits, wrap + mid + random_keys(nrec - 20, bits, rng, keep_out=out), absent)
    occ = occupied(case.table_keys(), bits)
    assert span(nslots - 4, 10, bits) <= occ and 6 not in occ and span(nslots // 2, 10, bits) <= occ
    return case


def case_f_empty():
    """an index of a sketch without minimizers (three contigs, every mx_off zero), asked for random keys, the all-ones key and 0"""
    rng = np.random.default_rng(699)
    case = Case("f-empty", rng, 10, [], [ALL_ONES, 0] + random_keys(30, 10, rng))
    assert case.n_records == 0 and not case.coff.any() and len(case.coff) == 4 and len(case.reads[2]) == 32
    return case


G_CONTIGS = [0, 65535, 65536, 69999]


def case_g():
    """g. contig ids above 65535: 70 000 contigs, thirty random keys each on contigs 0, 65535, 65536 and 69999, a read for each"""
    rng = np.random.default_rng(700)
    case = Case("g-contig-ids", rng, 10, random_keys(120, 10, rng), random_keys(20, 10, rng), n_ctg=70000, on=G_CONTIGS)
    assert len(case.reads[0]) == 5 and all(case.coff[c + 1] > case.coff[c] for c in G_CONTIGS)
    return case


ARRAY_CASES = {f"a-{n}": functools.partial(case_a, n) for n in (7, 8, 9, 10, 16, 40)}
ARRAY_CASES.update({f"b-{n}-at-{s}": functools.partial(case_b, n, s) for n, s in B_CLUSTERS})
ARRAY_CASES["b-seam12"] = case_b_seam
ARRAY_CASES["c-extreme-tags"] = case_c
ARRAY_CASES.update({"d-" + v: functools.partial(case_d, v) for v in D_VARIANTS})
ARRAY_CASES["e-dup-1024"] = functools.partial(case_e, 10)
ARRAY_CASES["e-dup-4096"] = functools.partial(case_e, 12)
ARRAY_CASES.update({f"f-{n}": functools.partial(case_f, n, b) for n, b in F_SIZES})
ARRAY_CASES["f-empty"] = case_f_empty
ARRAY_CASES["g-contig-ids"] = case_g


@functools.lru_cache(maxsize=None)
def array_case(name):
    """the case of that name, built once (the mock half and the GPU half share it and its expected records)"""
    return ARRAY_CASES[name]()


# ---------------------------------------------------------------- an index crafted round the minimizers of real sequence

ACGT = np.frombuffer(b"ACGT", np.uint8)
N_PICK, N_COLLIDE, N_SEAM = 32, 11, 4


class EmitCase:
    """For the lookups a sketch makes while it emits (Device.sketch(batch, k, w, index=ix)): hashes cannot be crafted from a sequence, so
    the index is crafted round the sequence.  Six random reads of 20 kb at k = 24 and the oracle's sketch of them; 32 of the read
    minimizers are in the index, on a contig of its own for every read, at the read's positions (so the reads map), 32 stay absent; each of the 64 gets
    eleven collider keys of its own home slot -- three of them with its own tag -- so its lookup walks a cluster of 11 or 12; the homes of
    at least four of the 64 lie in the last eight slots of the table."""

    def __init__(self, w, seed=900):
        rng = np.random.default_rng(seed + w)
        self.w = w
        self.seqs = [bytes(ACGT[rng.integers(0, 4, 20000)]) for _ in range(6)]
        off = np.zeros(len(self.seqs) + 1, np.uint64)
        np.cumsum([len(s) for s in self.seqs], out=off[1:])
        self.sketch = qoff, qh, qp, qs = oracle.sketch_batch(b"".join(self.seqs), off, K, w)
        self.rlen = np.array([len(s) for s in self.seqs], np.uint32)
        nrec = N_PICK + 2 * N_PICK * N_COLLIDE
        self.bits = bits = table_bits(nrec)
        assert bits == 11
        nslots = 1 << bits
        uniq, cnt = np.unique(qh, return_counts=True)
        once = set(int(h) for h in uniq[cnt == 1]) - {ALL_ONES}
        idx = [i for i in range(len(qh)) if int(qh[i]) in once]
        seam = [i for i in idx if home(int(qh[i]), bits) >= nslots - 8]
        assert len(idx) > 500 and len(seam) >= N_SEAM, (len(idx), len(seam))  # hundreds to pick from, enough at the table's end
        seam = seam[:2 * N_SEAM]
        rest = [i for i in rng.permutation(idx) if i not in set(seam)]
        picked = seam + [int(i) for i in rest[:2 * N_PICK - len(seam)]]
        present, absent = sorted(picked[0::2]), sorted(picked[1::2])  # the seam homes alternate between the two
        assert len(present) == len(absent) == N_PICK
        assert min(sum(1 for i in part if home(int(qh[i]), bits) >= nslots - 8) for part in (present, absent)) >= N_SEAM // 2
        read_of = np.searchsorted(qoff, np.arange(len(qh)), side="right") - 1
        colliders = []
        for i in picked:
            h = int(qh[i])
            own = keys_at(home(h, bits), bits, 3, rng, tag=tag(h), avoid=once | set(colliders))
            colliders += own + keys_at(home(h, bits), bits, N_COLLIDE - 3, rng, avoid=once | set(colliders) | set(own))
        colliders = [colliders[i] for i in rng.permutation(len(colliders))]
        # the colliders' contigs partly in front of the reads' contigs and partly behind them: where inserts land in record order, a
        # picked minimizer lies behind those of its colliders that came first -- at any depth of its cluster, not always at its home
        n_extra = -(-len(colliders) // PER_CTG)
        n_front = n_extra // 2 + 1
        n_ctg = len(self.seqs) + n_extra
        lens, counts = [], []
        ch, cp, cs = [], [], []

        def collider_contig(c):
            mine = colliders[c::n_extra]
            lens.append(CTG_LEN); counts.append(len(mine))
            ch.extend(mine); cp.extend(int(p) for p in np.sort(rng.choice(CTG_LEN - K, len(mine), replace=False)))
            cs.extend(int(s) for s in rng.integers(0, 2, len(mine)))

        for c in range(n_front):
            collider_contig(c)
        n_present = []
        for r in range(len(self.seqs)):  # in read order: positions increase within a contig
            mine = [i for i in present if read_of[i] == r]
            lens.append(20000); counts.append(len(mine)); n_present.append(len(mine))
            ch += [int(qh[i]) for i in mine]; cp += [int(qp[i]) for i in mine]; cs += [int(s) for s in rng.integers(0, 2, len(mine))]
        for c in range(n_front, n_extra):
            collider_contig(c)
        self.ctg_len = np.array(lens, np.uint32)
        assert len(ch) == nrec and table_bits(len(ch)) == bits
        assert len(counts) == n_ctg and 0 < n_front < n_extra
        self.coff = np.zeros(n_ctg + 1, np.uint64)
        np.cumsum(counts, out=self.coff[1:])
        self.ch, self.cp, self.cs = np.array(ch, np.uint64), np.array(cp, np.uint32), np.array(cs, np.uint8)
        occ = occupied(ch, bits)
        assert all(span(home(int(qh[i]), bits), N_COLLIDE, bits) <= occ for i in picked)
        # a batch of the present minimizers alone: every lookup hits
        hit_off = np.zeros(len(self.seqs) + 1, np.uint64)
        np.cumsum(n_present, out=hit_off[1:])
        self.all_hit = (hit_off, self.rlen, qh[present], qp[present], qs[present])
        oix = oracle.Index(self.ch, contig_ids(self.coff), self.cp, self.cs)
        self.index_size = len(oix)
        self.exp = oracle.map_reads(oix, self.ctg_len, qoff, self.rlen, qh, qp, qs, k=K, threads=0)
        self.found = sum(1 for h in qh if oix.lookup(int(h)) is not None)
        assert self.index_size == nrec and self.found == N_PICK == len(self.exp["hits"]) and len(self.exp["maps"]) >= 4


@functools.lru_cache(maxsize=None)
def emit_case(w):
    return EmitCase(w)
