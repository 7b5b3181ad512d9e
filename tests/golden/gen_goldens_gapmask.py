#!/usr/bin/env python3
"""Golden vectors for the gap filler's masking step and what follows it: the reference's own print_masked_sequences
(bin/ntlink_patch_gaps.py:346-389) and then its map_long_reads (:412-489), nothing wrapped, with the reference's PairInfo and
ScaffoldGaps, over UNMASKED scaffolds and reads made below.  Output: tests/golden/gen/gapmask_cases.json.gz (data only): the unmasked
records, the pairs with their chosen read and the cuts they hold before the call, the bytes of the two temporary files as the reference
wrote them, and per run -- `stringent` off and on -- every pair's five fields in dict order and every scaffold's two cuts at the end.

Same import recipe and the same `btllib` / `igraph` stubs as gen_goldens_gapcuts.py.  The conditions at the end of main() are what
tests/test_gap_mask.py relies on; if a gap misses one, change the gap, not the condition."""
import argparse
import gzip
import json
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
import oracle  # noqa: E402

K, W, Z = 20, 10, 1000
OUT = os.path.join(REPO, "tests", "golden", "gen", "gapmask_cases.json.gz")
ACGT = np.frombuffer(b"ACGT", np.uint8)


# ---------------------------------------------------------------- the btllib stub (as in gen_goldens_gapcuts.py)

class _Mx:
    def __init__(self, h, p, s):
        self.out_hash, self.pos, self.forward = int(h), int(p), bool(s)


class _Record:
    def __init__(self, num, name, seq, k, w):
        self.num, self.id, self.readlen = num, name, len(seq)
        self.minimizers = [_Mx(h, p, s) for h, p, s in zip(*oracle.sketch_seq(seq, k, w))]


class _Indexlr:
    def __init__(self, path, k, w, flags=0, threads=1):
        self._it = (_Record(i, name, seq, k, w) for i, (name, seq) in enumerate(oracle.read_fastx(path)))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def __iter__(self):
        return self._it

    def read(self):
        return next(self._it)


btllib = types.ModuleType("btllib")
btllib.Indexlr = _Indexlr
btllib.IndexlrFlag = types.SimpleNamespace(LONG_MODE=0)
sys.modules["btllib"] = btllib
sys.modules["igraph"] = types.ModuleType("igraph")
sys.path.insert(0, "/root/reference/bin")
import ntlink_patch_gaps  # noqa: E402  (the reference)


# ---------------------------------------------------------------- the gaps

def rand(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def revcomp(seq):
    return seq.upper().translate(bytes.maketrans(b"ACGTN", b"TGCAN"))[::-1]


def oriented(seq, sign):
    return seq.upper() if sign == "+" else revcomp(seq)


def mutate(rng, seq, rate):
    a = np.frombuffer(seq, np.uint8).copy()
    hit = np.flatnonzero((rng.random(len(a)) < rate) & np.isin(a, ACGT))
    a[hit] = ACGT[(np.searchsorted(ACGT, a[hit]) + rng.integers(1, 4, len(hit))) % 4]
    return a.tobytes()


def build(seed=7):
    """-> scaffolds {name: bytes}, reads {id: bytes}, pairs [[source, target, chosen read or None, the four preset cuts]], tags"""
    rng = np.random.default_rng(seed)
    scaffolds, reads, pairs, tags = {}, {}, [], []

    def scaffold(name, n, lower=None, n_run=None):
        seq = bytearray(rand(rng, n))
        if lower:
            seq[lower[0]:lower[1]] = bytes(seq[lower[0]:lower[1]]).lower()
        if n_run:
            seq[n_run[0]:n_run[1]] = b"N" * (n_run[1] - n_run[0])
        scaffolds[name] = bytes(seq)

    def end_cut(node, keep, is_source):
        """the cut that keeps `keep` bases of the end of `node` beside the gap"""
        length = len(scaffolds[node[:-1]])
        return length - keep if (node[-1] == "+") == is_source else keep

    def read_over(nodes, reach, own, flip, rate=0.0):
        """a read over the ends of the nodes beside their gaps (the middle nodes whole), `own` bases of its own between them"""
        parts = []
        for i, node in enumerate(nodes):
            seq = oriented(scaffolds[node[:-1]], node[-1])
            piece = seq[len(seq) - reach:] if i == 0 else (seq[:reach] if i == len(nodes) - 1 else seq)
            parts += [piece.replace(b"N", b"A"), rand(rng, own)]
        read = b"".join(parts[:-1])
        if rate:
            read = mutate(rng, read, rate)
        return revcomp(read) if flip else read

    def gap(tag, source, target, read_id, keep=(600, 600), read_cuts=None, cuts=None):
        sc, tc = cuts or (end_cut(source, keep[0], True), end_cut(target, keep[1], False))
        if read_id is None:
            pairs.append([source, target, None, None, None, None, None])
        else:
            sr, tr = read_cuts or (5, len(reads[read_id]) - 7)
            pairs.append([source, target, read_id, sc, sr, tc, tr])
        tags.append(tag)

    scaffold("sA", 2100)
    scaffold("sB", 1901, lower=(1500, 1700))
    scaffold("sC", 2400, n_run=(2100, 2130))            # an interior N run inside the end that is kept
    scaffold("sD", 1800, lower=(100, 400), n_run=(200, 260))
    scaffold("sE", 2000)
    scaffold("sF", 1700)
    scaffold("sG", 1150)                                 # the middle of a chain, spanned whole by one read
    scaffold("sH", 1600)
    scaffold("sI", 1500)
    scaffold("sJ", 1300)
    scaffold("sK", 1250, lower=(0, 1250))                # all lower case
    scaffold("sL", 1400)
    scaffold("sM", 1100)
    scaffold("sN", 1200)

    # the four sign combinations, reads forward and reverse-complemented, with and without substitutions
    reads["r_pp"] = read_over(["sA+", "sB+"], 500, 150, False)
    gap("plus_plus", "sA+", "sB+", "r_pp")
    reads["r_pm"] = read_over(["sC+", "sD-"], 550, 90, True, 0.03)
    gap("plus_minus", "sC+", "sD-", "r_pm", read_cuts=(len(reads["r_pm"]) - 3, 11))   # the cuts the other way round
    gap("no_read", "sB+", "sC+", None)                   # between two pairs with a read
    reads["r_mp"] = read_over(["sE-", "sF+"], 500, 200, False, 0.03)
    gap("minus_plus", "sE-", "sF+", "r_mp")
    reads["r_mm"] = read_over(["sB-", "sA-"], 450, 30, True)
    gap("minus_minus", "sB-", "sA-", "r_mm")
    # one read over F -> G -> H, chosen by both pairs: G is the target of one gap and the source of the next
    reads["r_chain"] = read_over(["sF+", "sG+", "sH+"], 500, 120, False)
    at_g = 500 + 120
    gap("chain_fg", "sF+", "sG+", "r_chain", keep=(600, 450), read_cuts=(3, at_g + 450))
    gap("chain_gh", "sG+", "sH+", "r_chain", keep=(450, 600), read_cuts=(at_g + 450, len(reads["r_chain"]) - 2))
    # a read whose two cuts are equal: fully masked, nothing maps
    reads["r_empty"] = read_over(["sI+", "sJ+"], 500, 100, False)
    gap("read_masked", "sI+", "sJ+", "r_empty", read_cuts=(400, 400))
    # scaffold cuts 0 and length: the whole source and the whole target are kept
    reads["r_whole"] = read_over(["sK+", "sL+"], 600, 80, True)
    gap("cut_0_and_len", "sK+", "sL+", "r_whole", cuts=(0, len(scaffolds["sL"])))
    # ... and the other two: nothing of either is kept
    reads["r_none"] = read_over(["sM+", "sN+"], 500, 80, False)
    gap("cut_len_and_0", "sM+", "sN+", "r_none", cuts=(len(scaffolds["sM"]), 0))
    # the scaffold ends are kept too short for the read's flanks: one side alone maps
    reads["r_short"] = read_over(["sJ-", "sI-"], 500, 100, False)
    gap("short_end", "sJ-", "sI-", "r_short", keep=(600, 15))
    return scaffolds, reads, pairs, tags


def run_reference(scaffolds, reads, pairs, stringent):
    """the two files the reference's print_masked_sequences writes and the end state its map_long_reads leaves behind them"""
    scaf = {name: ntlink_patch_gaps.ScaffoldGaps(seq.decode()) for name, seq in scaffolds.items()}
    rds = {rid: seq.decode() for rid, seq in reads.items()}
    info = {}
    for source, target, chosen, sc, sr, tc, tr in pairs:
        p = ntlink_patch_gaps.PairInfo(100)
        p.chosen_read, p.source_ctg_cut, p.source_read_cut, p.target_ctg_cut, p.target_read_cut = chosen, sc, sr, tc, tr
        info[(source, target)] = p
    assert len(info) == len(pairs)
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "g")
        args = argparse.Namespace(o=prefix, k=K, w=W, t=1, z=Z, x=0.0, sensitive=False, stringent=stringent)
        ntlink_patch_gaps.print_masked_sequences(scaf, rds, info, args)
        files = [open(prefix + suffix).read() for suffix in (".scaffolds.masked_temp.fa", ".reads.masked_temp.fa")]
        ntlink_patch_gaps.map_long_reads(info, scaf, args)
    state = {"stringent": stringent,
             "pairs": [[p.source_ctg_cut, p.source_read_cut, p.target_ctg_cut, p.target_read_cut, p.old_anchor_used] for p in info.values()],
             "scaffolds": {name: [s.five_prime_cut, s.three_prime_cut] for name, s in scaf.items()}}
    return files, state


def main():
    scaffolds, reads, pairs, tags = build()
    files, plain = run_reference(scaffolds, reads, pairs, False)
    files_again, strict = run_reference(scaffolds, reads, pairs, True)
    assert files == files_again
    at = {t: i for i, t in enumerate(tags)}
    chosen = [p for p in pairs if p[2] is not None]
    # all four sign combinations
    assert {(p[0][-1], p[1][-1]) for p in chosen} == {("+", "+"), ("+", "-"), ("-", "+"), ("-", "-")}
    # a pair without a chosen read between two with one
    g = at["no_read"]
    assert pairs[g][2] is None and pairs[g - 1][2] is not None and pairs[g + 1][2] is not None
    assert plain["pairs"][g] == [None, None, None, None, False]
    # a read whose two cuts are equal
    assert pairs[at["read_masked"]][4] == pairs[at["read_masked"]][6]
    # a scaffold cut of 0 and one equal to the length, kept whole and not at all
    g = at["cut_0_and_len"]
    assert pairs[g][3] == 0 and pairs[g][5] == len(scaffolds[pairs[g][1][:-1]])
    g = at["cut_len_and_0"]
    assert pairs[g][5] == 0 and pairs[g][3] == len(scaffolds[pairs[g][0][:-1]])
    # a scaffold that is the target of one gap and the source of the next; one read chosen by two pairs
    fg, gh = pairs[at["chain_fg"]], pairs[at["chain_gh"]]
    assert at["chain_gh"] == at["chain_fg"] + 1 and fg[1] == gh[0] and fg[2] == gh[2]
    five, three = plain["scaffolds"]["sG"]
    assert 0 < five < three < len(scaffolds["sG"]), "sG is cut at both ends"
    # lower case and an interior N run, inside ends that are kept
    scaf_file = files[0].split("\n")
    assert any(any(c in line for c in "acgt") for line in scaf_file if not line.startswith(">"))
    assert any("N" in line.strip("N") for line in scaf_file if not line.startswith(">"))
    # a gap that falls back to the old anchors and one that does not; stringent's None
    used = [p[4] for p, q in zip(plain["pairs"], pairs) if q[2] is not None]
    assert any(used) and not all(used), used
    for tag in ("plus_plus", "plus_minus", "minus_plus", "minus_minus", "chain_fg", "chain_gh", "cut_0_and_len"):
        assert plain["pairs"][at[tag]][4] is False, tag
    for tag in ("read_masked", "cut_len_and_0", "short_end"):
        assert plain["pairs"][at[tag]][4] is True and strict["pairs"][at[tag]][1] is None, tag
        assert plain["pairs"][at[tag]][:4] == pairs[at[tag]][3:], "a fallback leaves the pair's preset cuts"
    print(f"{len(pairs)} pairs, {len(chosen)} with a read, {sum(used)} fall back")
    doc = {"k": K, "w": W, "z": Z, "x": 0.0, "sensitive": False, "tags": tags,
           "scaffolds": [[n, s.decode()] for n, s in scaffolds.items()], "reads": [[i, s.decode()] for i, s in reads.items()],
           "pairs": pairs, "files": {"scaffolds": files[0], "reads": files[1]}, "sets": [plain, strict]}
    raw = json.dumps(doc, separators=(",", ":")).encode()
    with open(OUT, "wb") as fh, gzip.GzipFile(filename="", mode="wb", fileobj=fh, mtime=0) as gz:
        gz.write(raw)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) <= 1 << 20


if __name__ == "__main__":
    main()
