"""Inputs and expected records for the grouped map (Device.map_grouped, csrc/group_kernels.h): every read is looked up in the contigs of
its own group alone.  A case is a list of groups; a group is a set of arrays for sketch_from_arrays with what the oracle makes of it ON ITS
OWN (oracle.Index + oracle.map_reads on the group's slice); compose() concatenates the groups into the two sketches and the two offset
arrays and shifts the oracle's read and contig numbers to the global ones.  The crafted groups are index_cases.Case objects: keys of a
chosen home slot in a table of table_bits(records) bits -- group_table_bits restates exactly that rule (test_source_literals)."""
import functools

import numpy as np

import index_cases as ic
import oracle
from helpers import contig_ids

K = ic.K
ACGT = np.frombuffer(b"ACGT", np.uint8)


class Group:
    """coff u64[n_ctg + 1], ch/cp/cs, ctg_len; reads = (roff, rlen, rh, rp, rs); exp = the oracle's records of the group alone (None: made
    here); found = read minimizers the oracle's index of the group holds"""

    def __init__(self, name, coff, ch, cp, cs, ctg_len, reads, exp=None, found=None, **kw):
        self.name, self.coff, self.ch, self.cp, self.cs, self.ctg_len, self.reads = name, coff, ch, cp, cs, ctg_len, reads
        self.n = len(ch)
        if exp is None:
            exp, found = oracle_group(self, **kw)
        self.exp, self.found = exp, found


def oracle_group(g, **kw):
    roff, rlen, rh, rp, rs = g.reads
    oix = oracle.Index(g.ch, contig_ids(g.coff) if len(g.ch) else np.empty(0, np.uint32), g.cp, g.cs)
    kw.setdefault("k", K)
    exp = oracle.map_reads(oix, g.ctg_len if len(g.ctg_len) else np.zeros(1, np.uint32), roff, rlen, rh, rp, rs, threads=0, **kw)
    uniq, cnt = np.unique(g.ch, return_counts=True)
    found = int(np.isin(rh, uniq[cnt == 1]).sum())  # a hash twice among the group's contig minimizers is dropped for the group
    assert len(oix) == int((cnt == 1).sum())
    return exp, found


def from_case(case):
    exp, _size, found = case.expected()  # (found: by the oracle's own lookups)
    return Group(case.name, case.coff, case.ch, case.cp, case.cs, case.ctg_len, case.reads, exp, found)


class Composite:
    def __init__(self, name, groups, **kw):
        self.name, self.groups, self.kw = name, groups, kw
        self.cgo = np.zeros(len(groups) + 1, np.uint32)
        self.rgo = np.zeros(len(groups) + 1, np.uint32)
        coffs, roffs = [np.zeros(1, np.uint64)], [np.zeros(1, np.uint64)]
        maps, hits, pafs = [], [], []
        nc = nr = nmx_c = nmx_r = nhit = 0
        for i, g in enumerate(groups):
            roff, rlen, rh, rp, rs = g.reads
            coffs.append(g.coff[1:] + np.uint64(nmx_c)); roffs.append(roff[1:] + np.uint64(nmx_r))
            m, p = g.exp["maps"].copy(), g.exp["pafs"].copy()
            m["read"] += nr; m["ctg"] += nc; m["hit_off"] += nhit
            p["read"] += nr; p["ctg"] += nc
            maps.append(m); hits.append(g.exp["hits"]); pafs.append(p)
            nc += len(g.coff) - 1; nr += len(roff) - 1; nmx_c += g.n; nmx_r += len(rh); nhit += len(g.exp["hits"])
            self.cgo[i + 1], self.rgo[i + 1] = nc, nr
        cat = lambda arrs, dt: np.concatenate([np.asarray(a, dt) for a in arrs]) if arrs else np.empty(0, dt)
        self.coff, self.roff = np.concatenate(coffs), np.concatenate(roffs)
        self.ch, self.cp, self.cs = cat([g.ch for g in groups], np.uint64), cat([g.cp for g in groups], np.uint32), cat([g.cs for g in groups], np.uint8)
        self.ctg_len = cat([g.ctg_len for g in groups], np.uint32)
        self.rlen = cat([g.reads[1] for g in groups], np.uint32)
        self.rh, self.rp, self.rs = cat([g.reads[2] for g in groups], np.uint64), cat([g.reads[3] for g in groups], np.uint32), cat([g.reads[4] for g in groups], np.uint8)
        self.exp = {"maps": cat(maps, oracle.MAPPING_DT), "hits": cat(hits, oracle.HIT_DT), "pafs": cat(pafs, oracle.PAF_DT)}
        self.found = sum(g.found for g in groups)
        self.sizes = [g.n for g in groups]

    def expected_info(self, S):
        """where the sizing rule puts every group's table: LDS when 2 n + 2 <= S"""
        in_lds = sum(1 for n in self.sizes if 2 * n + 2 <= S)
        return in_lds, len(self.sizes) - in_lds


def empty_reads():
    return ic.Case._read_arrays([])


def no_contigs(name, seed, n_keys=30):
    """a group without contigs whose reads ask for random keys, the all-ones key and 0"""
    rng = np.random.default_rng(seed)
    toks = [(key, int(rng.integers(0, 2))) for key in [ic.ALL_ONES, 0] + ic.random_keys(n_keys, 10, rng)]
    return Group(name, np.zeros(1, np.uint64), np.empty(0, np.uint64), np.empty(0, np.uint32), np.empty(0, np.uint8), np.empty(0, np.uint32),
                 ic.Case._read_arrays([toks[:10], toks[10:]]))


def without_reads(case, name):
    return Group(name, case.coff, case.ch, case.cp, case.cs, case.ctg_len, empty_reads())


def plain(name, seed, n=60, extra_present=(), extra_absent=(), copies=None, bits=None):
    """n random keys (and the given ones) present, ten random keys (and the given ones) absent"""
    rng = np.random.default_rng(seed)
    nrec = n + len(extra_present) + sum(t for t, _ in (copies or {}).values())
    bits = bits or ic.table_bits(nrec)
    avoid = set(extra_present) | set(extra_absent) | set(copies or {})
    keys = [key for key in ic.random_keys(n + 20, bits, rng) if key not in avoid]
    return ic.Case(name, rng, bits, keys[:n] + list(extra_present), keys[n:n + 10] + list(extra_absent), copies)


def sized(n):
    """n records with a cluster of 10 of one home across the end of the group's own table and one of 10 in its middle"""
    bits = ic.table_bits(n)
    rng = np.random.default_rng(6000 + n)
    nslots = 1 << bits
    wrap, mid = ic._cluster(nslots - 4, bits, 10, rng), ic._cluster(nslots // 2, bits, 10, rng)
    out = [(nslots - 64, nslots), (0, 32), (nslots // 2 - 40, nslots // 2 + 40)]
    absent = ic._cluster_absent(nslots - 4, bits, wrap, rng) + ic._cluster_absent(nslots // 2, bits, mid, rng) + ic.random_keys(20, bits, rng)
    case = ic.Case(f"sized-{n}", rng, bits, wrap + mid + ic.random_keys(n - 20, bits, rng, keep_out=out), absent)
    occ = ic.occupied(case.table_keys(), bits)
    assert ic.span(nslots - 4, 10, bits) <= occ and 6 not in occ and ic.span(nslots // 2, 10, bits) <= occ
    return case


def _shared_keys(seed, n=12):
    return ic.random_keys(n, 10, np.random.default_rng(seed))


def case_a():
    """a. the same keys in two groups: found in both (one index over both groups would drop them)"""
    shared = _shared_keys(11)
    return [from_case(plain("a-first", 12, extra_present=shared)), from_case(plain("a-second", 13, extra_present=shared))]


def case_b():
    """b. a key twice in one group -- across two contigs, and inside one contig -- is absent there and present in both neighbours"""
    across, same = _shared_keys(21, 4), _shared_keys(22, 4)
    copies = {key: (2, "across") for key in across}
    copies.update({key: (2, "same") for key in same})
    return [from_case(plain("b-left", 23, extra_present=across + same)), from_case(plain("b-twice", 24, copies=copies)),
            from_case(plain("b-right", 25, extra_present=across + same))]


def case_c():
    """c. the keys of group A asked for by the reads of group B (and the other way round): not found"""
    a = plain("c-A", 31)
    b = plain("c-B", 32, extra_absent=a.table_keys()[:25])
    a2 = plain("c-A", 31, extra_absent=b.table_keys()[:25])
    return [from_case(a2), from_case(b)]


def case_d():
    """d. the all-ones key absent, once, twice in one contig, three times across contigs -- and once again behind them: present in some
    groups and dropped or absent in others at the same time; the key 0 beside it"""
    return [from_case(ic.case_d(v)) for v in ("absent", "once", "twice-in-one-contig", "three-times-across-contigs", "once", "alone")]


def case_e():
    """e. clusters of 9 and 20 keys of one home slot of a group's table, and a cluster across the end of the table"""
    return [from_case(ic._one_home("e-9", 5009, 9, 300, also_absent_at=(304, 308))),
            from_case(ic._one_home("e-20", 5020, 20, 700, also_absent_at=(710, 719))),
            from_case(ic.case_b(10, 1021)), from_case(ic.case_b(15, 1016))]


def case_f(S):
    """f. n = S/2 - 2, S/2 - 1 (the last that fits LDS), S/2 and 3 S (global), a small group between them"""
    return [from_case(sized(S // 2 - 2)), from_case(sized(S // 2 - 1)), from_case(plain("f-small", 61)), from_case(sized(S // 2)),
            from_case(sized(3 * S))]


def case_g():
    """g. a group without contigs, one without reads, one whose contigs have no minimizers, one with neither contigs nor reads"""
    nothing = Group("g-nothing", np.zeros(1, np.uint64), np.empty(0, np.uint64), np.empty(0, np.uint32), np.empty(0, np.uint8),
                    np.empty(0, np.uint32), empty_reads())
    return [no_contigs("g-no-contigs", 71), from_case(plain("g-plain", 72)), without_reads(plain("g-no-reads", 73), "g-no-reads"), nothing,
            from_case(ic.case_f_empty()), from_case(plain("g-last", 74))]


def case_h(n_empty):
    """h. contig numbers above 65535: a group of 70 000 contigs (hits on 0, 65535, 65536, 69999), then n_empty groups of one contig
    without minimizers and no read, then a plain group whose contigs are numbered 70 000 + n_empty and up"""
    one = Group("h-empty", np.zeros(2, np.uint64), np.empty(0, np.uint64), np.empty(0, np.uint32), np.empty(0, np.uint8),
                np.full(1, ic.CTG_LEN, np.uint32), empty_reads(), exp=oracle_empty(), found=0)
    return [from_case(ic.case_g())] + [one] * n_empty + [from_case(plain("h-last", 81))]


def oracle_empty():
    return {"maps": np.empty(0, oracle.MAPPING_DT), "hits": np.empty(0, oracle.HIT_DT), "pafs": np.empty(0, oracle.PAF_DT)}


CRAFTED = {"a": case_a, "b": case_b, "c": case_c, "d": case_d, "e": case_e, "g": case_g}


@functools.lru_cache(maxsize=None)
def crafted(name, arg=None):
    if name == "f":
        groups = case_f(arg)
    elif name == "h":
        groups = case_h(arg)
    else:
        groups = CRAFTED[name]()
    return Composite(name, groups, k=K)


# ---------------------------------------------------------------- random sequence

def _mutate(seq, rate, rng):
    seq = seq.copy()
    hit = rng.random(len(seq)) < rate
    seq[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    return seq


def _sketch_group(name, contigs, reads, k, w, **kw):
    def arrays(seqs):
        if not seqs:
            return np.zeros(1, np.uint64), np.empty(0, np.uint64), np.empty(0, np.uint32), np.empty(0, np.uint8)
        off = np.zeros(len(seqs) + 1, np.uint64)
        np.cumsum([len(s) for s in seqs], out=off[1:])
        return oracle.sketch_batch(b"".join(s.tobytes() for s in seqs), off, k, w)
    coff, ch, cp, cs = arrays(contigs)
    roff, rh, rp, rs = arrays(reads)
    return Group(name, coff, ch, cp, cs, np.array([len(s) for s in contigs], np.uint32),
                 (roff, np.array([len(s) for s in reads], np.uint32), rh, rp, rs), k=k, **kw)


@functools.lru_cache(maxsize=None)
def random_case(n_groups, k, w, seed=2024):
    """1 .. 3 contigs and 0 .. 3 reads per group, pieces of 200 .. 6000 random bases; a read is the end of one contig, some bases of its
    own and the start of the next contig, with 5 % substitutions; every tenth group has three contigs of 4000 .. 6000 bases (more
    minimizers than half an LDS table holds at either window)"""
    rng = np.random.default_rng(seed + 31 * k + w)
    groups = []
    for g in range(n_groups):
        large = g % 10 == 3
        n_ctg = 3 if large else int(rng.integers(1, 4))
        contigs = [ACGT[rng.integers(0, 4, int(rng.integers(4000, 6001) if large else rng.integers(200, 1501)))] for _ in range(n_ctg)]
        reads = []
        for _ in range(int(rng.integers(0, 4))):
            a = contigs[int(rng.integers(0, n_ctg))]
            b = contigs[int(rng.integers(0, n_ctg))]
            piece = np.concatenate([a[-int(rng.integers(100, 2500)):], ACGT[rng.integers(0, 4, int(rng.integers(0, 400)))],
                                    b[:int(rng.integers(100, 2500))]])
            reads.append(_mutate(piece, 0.05, rng)[:6000])
        groups.append(_sketch_group(f"r{g}", contigs, reads, k, w, z=500))
    return Composite(f"random-k{k}-w{w}", groups, k=k, z=500)
