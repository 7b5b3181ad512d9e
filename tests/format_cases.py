"""Crafted map results for the text of <prefix>.verbose_mapping.tsv and <prefix>.paf: the device formatter (csrc/format_kernels.h:
fmt_len_kernel, fmt_fill_kernel behind ntl_mapres_format), the dense copy (map_nhits_kernel, the scan, map_densify_kernel behind
ntl_mapres_download) and the host writers (csrc/ntl_io.cpp: Out::u32, Out::u64 behind ntl_write_verbose / ntl_write_paf).

Records that come out of the mapper have positions of five or six digits and hit regions wherever the gather put them.  Here the
records are chosen and handed to the device as they are (Device.mapres_from_host): every digit count on both sides of every power of
ten up to 2^32 - 1, hit regions with unused slots in front of, between and behind them, mappings of 1 .. 1000 hits round the 256
threads of a block, record counts that size the grid by the hits, by the mappings and by the PAF records, names of 0 .. 255 bytes.

A Batch holds the input (maps whose hit_off index `slots`, the slot array, pafs, the name tables and lengths), its dense restatement
made here in NumPy (hit_off = the running sum of n_hits, the hits gathered from their regions) and the expected text: plain Python
integer formatting (oracle.format_verbose / oracle.format_paf) of the dense records.  Nothing here comes from the code under test.
An unused slot holds FILL (both positions 2^32 - 1, both strands 1): a hit read from a wrong slot changes the text's length."""
import functools

import numpy as np

import oracle
from ntlink_amd.capi import HIT_DT, MAPPING_DT, PAF_DT

M32 = (1 << 32) - 1
FILL = (M32, M32, 1, 1, (0, 0))
# both sides of every power of ten, of 2^31 and the end of the range
V = [0] + [x for j in range(1, 10) for x in (10 ** j - 1, 10 ** j)] + [(1 << 31) - 1, 1 << 31, M32]
STRANDS = ((1, 1), (1, 0), (0, 1), (0, 0))
PAF_FIELDS = ("q_start", "q_end", "t_start", "t_end", "n_hits")
LONGEST = 255


def digits(v):
    return len(str(int(v)))


def verbose_bound(n_hits, n_maps, names2):
    """the bytes ntl_mapres_format allows the verbose text of a batch: a token and its separator are at most 27 bytes, a header two
    names, a count of at most ten digits, three tabs (16 with slack); names2 = the longest read name + the longest contig name"""
    return n_hits * 27 + n_maps * (names2 + 16)


def paf_bound(n_pafs, names2):
    """... and the PAF text: two names, ten numbers of at most eleven bytes with their tabs, strand, tabs, 255 and the newline"""
    return n_pafs * (names2 + 126)


class Batch:
    """mappings: [(read, ctg, [(ctg_pos, read_pos, ctg_strand, read_strand), ...]), ...]; pafs: [(read, ctg, q_start, q_end, t_start,
    t_end, n_hits, strand), ...]; lead: unused slots in front of the first region; gaps: unused slots behind region m (cycled);
    slack: unused slots behind the last region"""

    def __init__(self, name, read_names, read_len, ctg_names, ctg_len, mappings, pafs, lead=0, gaps=(0,), slack=0):
        self.name = name
        self.read_names, self.ctg_names = list(read_names), list(ctg_names)
        self.read_len, self.ctg_len = np.array(read_len, np.uint32), np.array(ctg_len, np.uint32)
        assert len(self.read_len) == len(self.read_names) and len(self.ctg_len) == len(self.ctg_names)
        self.maps = np.zeros(len(mappings), MAPPING_DT)
        at, regions = lead, []
        for m, (read, ctg, hits) in enumerate(mappings):
            assert len(hits) > 0 and 0 <= read < len(self.read_names) and 0 <= ctg < len(self.ctg_names)
            self.maps[m] = (read, ctg, len(hits), 0, at)
            regions.append((at, hits))
            at += len(hits) + (gaps[m % len(gaps)] if m + 1 < len(mappings) else 0)
        self.slots = np.full(at + slack, np.array(FILL, HIT_DT), HIT_DT)
        for off, hits in regions:
            self.slots[off:off + len(hits)] = np.array([(c, r, cs, rs, (0, 0)) for c, r, cs, rs in hits], HIT_DT)
        self.pafs = np.array([tuple(p) for p in pafs], PAF_DT) if len(pafs) else np.zeros(0, PAF_DT)
        assert all(0 <= int(r) < len(self.read_names) for r in self.pafs["read"]) and all(0 <= int(c) < len(self.ctg_names) for c in self.pafs["ctg"])
        assert (self.pafs["t_end"] >= self.pafs["t_start"]).all(), "the mapper's guarantee (map_kernels.h): t_end >= t_start"
        self.n_unused = len(self.slots) - sum(len(h) for _r, _c, h in mappings)
        # the dense restatement: running sums and a gather, from the arrays that go to the device
        n = self.maps["n_hits"].astype(np.int64)
        doff = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        src = np.concatenate([np.arange(o, o + k) for o, k in zip(self.maps["hit_off"].astype(np.int64), n)]) if len(n) else np.zeros(0, np.int64)
        dmaps = self.maps.copy()
        dmaps["hit_off"] = doff[:-1]
        self.dense = {"maps": dmaps, "hits": self.slots[src].copy(), "pafs": self.pafs.copy()}
        flat = [h for _r, _c, hits in mappings for h in hits]
        assert [tuple(x)[:4] for x in self.dense["hits"].tolist()] == [tuple(h) for h in flat], "the gather restates the mappings' own hits"
        self._text = None

    @property
    def names2(self):
        return max((len(n.encode()) for n in self.read_names), default=0) + max((len(n.encode()) for n in self.ctg_names), default=0)

    def text(self):
        """(verbose bytes, PAF bytes) by the oracle, made once"""
        if self._text is None:
            v = oracle.format_verbose(self.dense, self.read_names, self.ctg_names).encode()
            p = oracle.format_paf(self.dense, self.read_names, self.read_len, self.ctg_names, self.ctg_len).encode()
            self._text = (v, p)
        return self._text

    def numbers(self):
        """every number the two texts print, by field"""
        h, p = self.dense["hits"], self.pafs
        out = {"ctg_pos": h["ctg_pos"], "read_pos": h["read_pos"], "map_n_hits": self.maps["n_hits"]}
        out.update({f: p[f] for f in PAF_FIELDS})
        out["read_len"], out["ctg_len"] = self.read_len[p["read"].astype(np.int64)], self.ctg_len[p["ctg"].astype(np.int64)]
        out["span"] = p["t_end"].astype(np.int64) - p["t_start"].astype(np.int64)
        return {f: [int(x) for x in a] for f, a in out.items()}


def _names(prefix, n):
    return [f"{prefix}{i}" for i in range(n)]


# ---------------------------------------------------------------- the digit batch

def digit_batch():
    """Read i and contig i have the length V[i]; read and contig len(V) are the fixed ones of the records that vary another field.
    Mapping i holds (v, v), (v, 0), (0, v) for v = V[i], the strands cycling; one more mapping holds them all again in one long line.
    PAF: every field takes every v while the others stay fixed (t_start below a t_end of 2^32 - 1, t_end above a t_start of 0: the
    spans are 2^32 - 1 - v and v), every span again at the top of the range (t_end = 2^32 - 1), and equal ends there."""
    nv = len(V)
    lens = V + [12345]
    mappings, k = [], 0
    for i, v in enumerate(V):
        hits = []
        for c, r in ((v, v), (v, 0), (0, v)):
            hits.append((c, r) + STRANDS[k % 4])
            k += 1
        mappings.append((i, nv - 1 - i, hits))
    mappings.append((nv, nv, [(c, r) + STRANDS[(j + 1) % 4] for j, (c, r) in enumerate((x, y) for v in V for x, y in ((v, v), (v, 0), (0, v)))]))
    base = dict(q_start=1, q_end=22, t_start=0, t_end=M32, n_hits=333)
    pafs, k = [], 0
    for f in PAF_FIELDS:
        for v in V:
            d = dict(base, **{f: v})
            pafs.append((nv, nv, d["q_start"], d["q_end"], d["t_start"], d["t_end"], d["n_hits"], k % 2))
            k += 1
    for i in range(nv):  # read_len[read] and ctg_len[ctg] take every v
        pafs.append((i, nv, 1, 22, 4444, 55555, 333, i % 2))
        pafs.append((nv, i, 1, 22, 4444, 55555, 333, (i + 1) % 2))
    for s in V:  # the spans again, subtracted from the largest t_end; and a span of 0 at every v
        pafs.append((nv, nv, 1, 22, M32 - s, M32, 333, 1))
        pafs.append((nv, nv, 1, 22, s, s, 333, 0))
    b = Batch("digits", _names("read", nv + 1), lens, _names("ctg", nv + 1), lens, mappings, pafs, lead=3, gaps=(2, 0, 65), slack=9)
    # coverage, on the input alone
    toks = {digits(c) + digits(r) + 6 for _rd, _cg, hits in mappings for c, r, _a, _b in hits}
    assert 8 in toks and 26 in toks, toks
    num = b.numbers()
    for f in ("ctg_pos", "read_pos", "read_len", "ctg_len", "span") + PAF_FIELDS:
        assert {digits(x) for x in num[f]} == set(range(1, 11)), f
        assert set(V) <= set(num[f]), f
    assert set(V) <= set(num["span"]) and {(cs, rs) for _r, _c, hits in mappings for _x, _y, cs, rs in hits} == set(STRANDS)
    return b


# ---------------------------------------------------------------- random numbers of every digit count

def draw(rng, n):
    """n numbers, the digit count 1 .. 10 uniform, the value uniform among those of that count, clipped to 2^32 - 1"""
    d = rng.integers(1, 11, n)
    lo = np.where(d == 1, 0, 10 ** (d - 1).astype(np.int64))
    hi = 10 ** d.astype(np.int64) - 1
    return np.minimum(lo + (rng.random(n) * (hi - lo + 1)).astype(np.int64), M32)


def _hits(rng, n):
    c, r, s = draw(rng, n), draw(rng, n), rng.integers(0, 2, (n, 2))
    return [(int(c[i]), int(r[i]), int(s[i][0]), int(s[i][1])) for i in range(n)]


def _pafs(rng, n, n_reads, n_ctgs):
    """t_end >= t_start: one of the two and the span are drawn, the other follows (upwards to at most 2^32 - 1, downwards to at least 0)"""
    x, span, up = draw(rng, n), draw(rng, n), rng.integers(0, 2, n).astype(bool)
    t = np.stack([np.where(up, x, x - np.minimum(x, span)), np.where(up, np.minimum(x + span, M32), x)])
    q, h = np.stack([draw(rng, n), draw(rng, n)]), draw(rng, n)
    return [(int(rng.integers(0, n_reads)), int(rng.integers(0, n_ctgs)), int(q[0][i]), int(q[1][i]), int(t[0][i]), int(t[1][i]), int(h[i]),
             int(rng.integers(0, 2))) for i in range(n)]


HIT_COUNTS = (1, 9, 10, 11, 99, 100, 101, 255, 256, 257, 999, 1000)


def hit_count_batch():
    """mappings of exactly HIT_COUNTS hits: the header's count of one to four digits, the line's newline behind hit 255, 256 and 257
    of a mapping; the first region starts at slot 7, the regions lie 1, 63, 64, 300 and 0 slots apart, 50 unused slots at the end"""
    rng = np.random.default_rng(9100)
    mappings = [(i % 5, (3 * i) % 4, _hits(rng, n)) for i, n in enumerate(HIT_COUNTS)]
    b = Batch("hit-counts", _names("r", 5), draw(rng, 5), _names("c", 4), draw(rng, 4), mappings, _pafs(rng, 7, 5, 4), lead=7,
              gaps=(1, 63, 64, 300, 0), slack=50)
    assert b.maps["n_hits"].tolist() == list(HIT_COUNTS) and int(b.maps["hit_off"][0]) == 7
    between = (b.maps["hit_off"][1:] - b.maps["hit_off"][:-1] - b.maps["n_hits"][:-1]).tolist()
    assert {1, 63, 64, 300} <= set(between) and len(b.slots) == int(b.maps["hit_off"][-1]) + 1000 + 50
    return b


# ---------------------------------------------------------------- shapes

def shape_batch(which):
    rng = np.random.default_rng(9200 + len(which))
    rn, cn = _names("rd", 6), _names("cg", 5)
    rl, cl = draw(rng, 6), draw(rng, 5)

    def one_hit_maps(n):
        return [(i % 6, i % 5, _hits(rng, 1)) for i in range(n)]
    kw = dict(lead=2, gaps=(0, 3, 1), slack=4)
    if which == "empty":  # n_maps = 0 with n_pafs = 0 (slots there are, none used)
        mappings, pafs = [], []
    elif which == "one-mapping-one-hit":
        mappings, pafs = one_hit_maps(1), _pafs(rng, 1, 6, 5)
    elif which == "one-mapping-257-hits":
        mappings, pafs = [(5, 4, _hits(rng, 257))], _pafs(rng, 2, 6, 5)
    elif which in ("255-mappings", "256-mappings", "257-mappings"):
        n = int(which.split("-")[0])
        mappings, pafs = one_hit_maps(n), _pafs(rng, n // 2, 6, 5)
    elif which == "257-mappings-no-paf":  # ... and the regions adjacent, no unused slot anywhere
        mappings, pafs, kw = one_hit_maps(257), [], {}
    elif which == "600-pafs":  # the grid is sized by the PAF records
        mappings, pafs = one_hit_maps(1), _pafs(rng, 600, 6, 5)
    elif which == "5000-hits":  # ... by the hits
        mappings, pafs = [(0, 0, _hits(rng, 1)), (1, 1, _hits(rng, 2500)), (2, 2, _hits(rng, 2499))], _pafs(rng, 2, 6, 5)
    else:  # the same read and contig named again and again, the last read and the last contig of the tables
        assert which == "repeated-names"
        mappings = [(5, 4, _hits(rng, 2)), (5, 4, _hits(rng, 1)), (0, 4, _hits(rng, 3)), (5, 4, _hits(rng, 1)), (5, 0, _hits(rng, 2)), (5, 4, _hits(rng, 4))]
        pafs = [(5, 4) + p[2:] for p in _pafs(rng, 3, 6, 5)] + [(0, 4) + p[2:] for p in _pafs(rng, 1, 6, 5)] + [(5, 4) + p[2:] for p in _pafs(rng, 2, 6, 5)]
    return Batch("shape-" + which, rn, rl, cn, cl, mappings, pafs, **kw)


SHAPES = ("empty", "one-mapping-one-hit", "one-mapping-257-hits", "255-mappings", "256-mappings", "257-mappings", "257-mappings-no-paf",
          "600-pafs", "5000-hits", "repeated-names")


# ---------------------------------------------------------------- names

NAME_BYTES = (0, 1, 15, 16, 17, LONGEST)


def name_batch():
    """read and contig names of NAME_BYTES bytes, one of two- and three-byte UTF-8 characters, one with a space; every read name beside
    every contig name in a header and in a PAF line"""
    rng = np.random.default_rng(9300)
    rn = ["R" * n for n in NAME_BYTES] + ["léa_читать_讀", "read one"]
    cn = ["c" * n for n in NAME_BYTES] + ["ctg_ß_контиг_重", "contig 7 x"]
    assert [len(n.encode()) for n in rn[:6]] == list(NAME_BYTES) and max(rn[6].encode()) >= 0x80 and max(cn[6].encode()) >= 0x80
    pairs = [(r, c) for r in range(len(rn)) for c in range(len(cn))]
    mappings = [(r, c, _hits(rng, 1 + (r + c) % 3)) for r, c in pairs]
    pafs = [(r, c) + p[2:] for (r, c), p in zip(pairs, _pafs(rng, len(pairs), 1, 1))]
    return Batch("names", rn, draw(rng, len(rn)), cn, draw(rng, len(cn)), mappings, pafs, lead=1, gaps=(5, 0), slack=2)


# ---------------------------------------------------------------- random

def random_batch():
    """700 mappings of 1 .. 13 hits, 400 PAF records, 0 .. 40 unused slots between the regions"""
    rng = np.random.default_rng(9400)
    rn = [f"read_{i}/" + "x" * int(rng.integers(0, 30)) for i in range(90)]
    cn = [f"ctg{i:04d}" + "y" * int(rng.integers(0, 12)) for i in range(40)]
    mappings = [(int(rng.integers(0, 90)), int(rng.integers(0, 40)), _hits(rng, int(rng.integers(1, 14)))) for _ in range(700)]
    b = Batch("random", rn, draw(rng, 90), cn, draw(rng, 40), mappings, _pafs(rng, 400, 90, 40), lead=int(rng.integers(1, 41)),
              gaps=tuple(int(g) for g in rng.integers(0, 41, 699)), slack=int(rng.integers(1, 41)))
    assert len(b.maps) == 700 and 4500 < len(b.dense["hits"]) < 5500 and len(b.pafs) == 400 and b.n_unused > 700
    num = b.numbers()
    num["t_start, t_end"] = num["t_start"] + num["t_end"]  # one of the two is drawn, the other follows it: counted together
    for f in ("ctg_pos", "read_pos", "q_start", "q_end", "n_hits", "t_start, t_end"):
        count = np.bincount([digits(x) for x in num[f]], minlength=11)
        assert (count[1:] >= 20).all(), (f, count)
    return b


# ---------------------------------------------------------------- everything at its largest

def all_max_batch():
    """every position, length and PAF field 2^32 - 1, every name 255 bytes: the longest text a batch of these counts can have"""
    rn, cn = ["r" * LONGEST, "s" * LONGEST], ["C" * LONGEST, "D" * LONGEST]
    mappings = [(m % 2, (m + 1) % 2, [(M32, M32) + STRANDS[(m + j) % 4] for j in range(n)]) for m, n in enumerate((1, 3, 10, 20))]
    pafs = [(i % 2, i // 2, M32, M32, M32, M32, M32, i % 2) for i in range(4)]
    b = Batch("all-max", rn, [M32, M32], cn, [M32, M32], mappings, pafs, lead=5, gaps=(3,), slack=6)
    assert b.names2 == 2 * LONGEST
    # the PAF bound below the verbose one: with NTL_FORMAT_MAX_TEXT one above the verbose bound, both texts are made
    assert paf_bound(4, b.names2) <= verbose_bound(34, 4, b.names2)
    return b


BATCHES = {"digits": digit_batch, "hit-counts": hit_count_batch}
BATCHES.update({"shape-" + s: functools.partial(shape_batch, s) for s in SHAPES})
BATCHES.update({"names": name_batch, "random": random_batch, "all-max": all_max_batch})


@functools.lru_cache(maxsize=None)
def batch(name):
    """the batch of that name, built once (the mock half and the GPU half share it and its expected text)"""
    b = BATCHES[name]()
    assert b.name == name
    return b
