#!/usr/bin/env python3
"""Golden vectors for ntlink_amd.gapfill.map_long_reads: the reference's whole map_long_reads (bin/ntlink_patch_gaps.py:412-489), nothing
wrapped, with the reference's own PairInfo and ScaffoldGaps, over the 64 gaps of tests/golden/gen/gapmap_cases.json.gz and the gaps
crafted below for the branches those do not reach.  Output: tests/golden/gen/gapcut_cases.json.gz (data only): the crafted records (the
64 are read from the other fixture, not repeated), the values every pair's four cuts are preset to (so that a fallback shows in the
result), and per run -- `stringent` off and on -- every pair's five fields in file order and every scaffold's two cuts at the end.

Same import recipe and the same `btllib` / `igraph` stubs as gen_goldens_gapmap.py.  A second, instrumented run per setting records what
assess_accepted_anchor_contigs is given and returns; it serves the conditions at the end of main() alone (which branch every gap takes),
and its end state must equal the plain run's.  If a crafted gap misses its branch, change the gap, not the condition."""
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
BASE = os.path.join(REPO, "tests", "golden", "gen", "gapmap_cases.json.gz")
OUT = os.path.join(REPO, "tests", "golden", "gen", "gapcut_cases.json.gz")
CRAFTED = ["mixed_strands", "transposed", "single_hit", "chain_ab", "chain_bc"]
ACGT = np.frombuffer(b"ACGT", np.uint8)


# ---------------------------------------------------------------- the btllib stub (as in gen_goldens_gapmap.py)

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
    return seq.translate(bytes.maketrans(b"ACGTN", b"TGCAN"))[::-1]


def common(a, b):
    """minimizers of a whose hash is one of b's that occurs once"""
    hb, cnt = np.unique(oracle.sketch_seq(b, K, W)[0], return_counts=True)
    return int(np.isin(oracle.sketch_seq(a, K, W)[0], hb[cnt == 1]).sum())


def preset(g):
    """what pair g's four cuts hold before the call: source_ctg_cut, source_read_cut, target_ctg_cut, target_read_cut"""
    return [100 + 7 * g, 3 + g, 200 + 5 * g, 1000 + g]


def crafted_gaps(first, seed=11):
    """error-free reads; a source record is N-masked in front of its flank, a target record behind it"""
    rng = np.random.default_rng(seed)
    scaffolds, reads, tags = [], [], []

    def add(tag, sname, src, tname, tgt, read):
        g = first + len(reads)
        scaffolds.extend([(f"{sname}_source", src), (f"{tname}_target", tgt)])
        reads.append((f"{tag}-{g}__{sname}__{tname}", read))
        tags.append(tag)

    def ends(n_src=700, n_tgt=700):
        return rand(rng, n_src), rand(rng, n_tgt)

    # the middle third of the source flank reverse-complemented in the read: both strands among the source's hits
    sf, tf = ends(900)
    add("mixed_strands", "mixS+", b"N" * 500 + sf, "mixT+", tf + b"N" * 500,
        sf[:300] + revcomp(sf[300:600]) + sf[600:] + rand(rng, 150) + tf[:500])
    # two segments of the target flank in the other order in the read: one strand, positions up and down
    sf, tf = ends(700, 1000)
    add("transposed", "trS-", b"N" * 400 + sf, "trT+", tf + b"N" * 700,
        sf[-500:] + rand(rng, 120) + tf[:250] + tf[500:750] + tf[250:500] + tf[750:])
    # the shortest start of the target flank that, behind the read's own bases, shares exactly one minimizer with the flank
    sf, tf = ends()
    own = rand(rng, 100)
    reach = next(n for n in range(K, 200) if common(own + tf[:n] + b"N", tf) == 1)
    add("single_hit", "oneS+", b"N" * 600 + sf, "oneT-", tf + b"N" * 600, revcomp(sf[-450:] + own + tf[:reach] + b"N" * 300))
    # A -> B -> C: B is the target of one gap (a 5' cut) and the source of the next (a 3' cut), masked at its middle in both records
    a, b, c = rand(rng, 1500), rand(rng, 2400), rand(rng, 1500)
    add("chain_ab", "chA+", b"N" * 700 + a[700:], "chB+", b[:1200] + b"N" * 1200, a[-600:] + rand(rng, 200) + b[:600])
    add("chain_bc", "chB+", b"N" * 1200 + b[1200:], "chC+", c[:800] + b"N" * 700, b[-600:] + rand(rng, 200) + c[:600])
    assert tags == CRAFTED
    return scaffolds, reads, tags


def name_of(record_id):
    return record_id.rsplit("_", 1)[0].strip("+-")


def run_reference(scaffolds, reads, stringent, instrumented):
    """the end state of the reference's map_long_reads over the two files; with `instrumented` also what every gap's
    get_accepted_anchor_contigs and assess_accepted_anchor_contigs returned"""
    lengths = {}
    for sid, seq in scaffolds:
        assert lengths.setdefault(name_of(sid), len(seq)) == len(seq)
    scaf = {name: ntlink_patch_gaps.ScaffoldGaps("N" * length) for name, length in lengths.items()}
    pairs = {}
    for g, (rid, _seq) in enumerate(reads):
        p = ntlink_patch_gaps.PairInfo(100)
        p.source_ctg_cut, p.source_read_cut, p.target_ctg_cut, p.target_read_cut = preset(g)
        pairs[tuple(rid.split("__")[1:])] = p
    assert len(pairs) == len(reads)
    seen = []
    real_get, real_assess = ntlink_patch_gaps.ntlink_utils.get_accepted_anchor_contigs, ntlink_patch_gaps.assess_accepted_anchor_contigs

    def get(*a):
        out = real_get(*a)
        seen.append({"accepted": len(out[0]), "n_hits": [len(run.hits) for run in out[0].values()]})
        return out

    def assess(accepted, source_ori, source_scaf, target_ori, target_scaf):
        out = real_assess(accepted, source_ori, source_scaf, target_ori, target_scaf)
        seen[-1].update(src=(source_ori, out[0], out[1]), tgt=(target_ori, out[3], out[4]))
        return out

    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "g")
        for path, recs in ((prefix + ".scaffolds.masked_temp.fa", scaffolds), (prefix + ".reads.masked_temp.fa", reads)):
            with open(path, "wb") as fh:
                for rid, seq in recs:
                    fh.write(b">" + rid.encode() + b"\n" + seq + b"\n")
        args = argparse.Namespace(o=prefix, k=K, w=W, t=1, z=Z, x=0.0, sensitive=False, stringent=stringent)
        if instrumented:
            ntlink_patch_gaps.ntlink_utils.get_accepted_anchor_contigs, ntlink_patch_gaps.assess_accepted_anchor_contigs = get, assess
        try:
            ntlink_patch_gaps.map_long_reads(pairs, scaf, args)
        finally:
            ntlink_patch_gaps.ntlink_utils.get_accepted_anchor_contigs, ntlink_patch_gaps.assess_accepted_anchor_contigs = real_get, real_assess
    state = {"stringent": stringent,
             "pairs": [[p.source_ctg_cut, p.source_read_cut, p.target_ctg_cut, p.target_read_cut, p.old_anchor_used] for p in pairs.values()],
             "scaffolds": {name: [s.five_prime_cut, s.three_prime_cut] for name, s in scaf.items()}}
    return state, seen, lengths


def main():
    with gzip.open(BASE, "rt") as fh:
        base = json.load(fh)
    assert base["k"] == K and base["w"] == W and len(base["reads"]) == 64
    more_scaffolds, more_reads, more_tags = crafted_gaps(len(base["reads"]))
    scaffolds = [(i, s.encode()) for i, s in base["scaffolds"]] + more_scaffolds
    reads = [(i, s.encode()) for i, s in base["reads"]] + more_reads
    tags = base["tags"] + more_tags
    sets = []
    for stringent in (False, True):
        state, _none, lengths = run_reference(scaffolds, reads, stringent, False)
        again, seen, _ = run_reference(scaffolds, reads, stringent, True)
        assert again == state and len(seen) == len(reads), "the instrumented run changes nothing"
        sets.append(state)
    plain, strict = sets
    at = {t: tags.index(t) for t in CRAFTED + ["equal_names"]}
    two = [g for g, s in enumerate(seen) if s["accepted"] == 2]
    valid = [g for g in two if None not in (seen[g]["src"][1], seen[g]["tgt"][1]) and seen[g]["src"][2] and seen[g]["tgt"][2]]
    print(f"{len(reads)} gaps: {len(two)} with two accepted contigs, {len(valid)} with new cuts")
    # the situations A-D of :276-288 (the contig's sign, the read-based orientation), for a source and for a target
    for side in ("src", "tgt"):
        got = {(seen[g][side][0], seen[g][side][1]) for g in valid}
        assert got == {("+", "+"), ("+", "-"), ("-", "-"), ("-", "+")}, (side, got)
    # every exit: new cuts, the fallback, stringent's None
    for g in range(len(reads)):
        new = g in valid
        assert plain["pairs"][g][4] == (not new) and strict["pairs"][g][4] is False
        assert (strict["pairs"][g][1] is None and strict["pairs"][g][3] is None) == (not new)
        if not new:
            assert plain["pairs"][g][:4] == preset(g), "a fallback leaves the pair's preset cuts"
    assert valid and len(valid) < len(reads) and any(g not in two for g in range(len(reads)))
    mixed, positions, single = at["mixed_strands"], at["transposed"], at["single_hit"]
    assert seen[mixed]["accepted"] == 2 and seen[mixed]["src"][1] is None and seen[mixed]["tgt"][1] == "+"
    assert seen[positions]["accepted"] == 2 and seen[positions]["tgt"][1] == "+" and seen[positions]["tgt"][2] is False and seen[positions]["src"][2]
    assert single in valid and 1 in seen[single]["n_hits"], seen[single]
    ab, bc = at["chain_ab"], at["chain_bc"]
    assert ab in valid and bc in valid
    five, three = plain["scaffolds"]["chB"]
    assert five == plain["pairs"][ab][2] > 0 and three == plain["pairs"][bc][0] < lengths["chB"] and five < three
    assert seen[at["equal_names"]]["accepted"] <= 1 and plain["pairs"][at["equal_names"]][4] is True
    doc = {"k": K, "w": W, "z": Z, "x": 0.0, "sensitive": False, "base": os.path.basename(BASE), "tags": tags,
           "scaffolds": [[i, s.decode()] for i, s in more_scaffolds], "reads": [[i, s.decode()] for i, s in more_reads],
           "lengths": lengths, "preset": [preset(g) for g in range(len(reads))], "sets": sets}
    raw = json.dumps(doc, separators=(",", ":")).encode()
    with open(OUT, "wb") as fh, gzip.GzipFile(filename="", mode="wb", fileobj=fh, mtime=0) as gz:
        gz.write(raw)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) <= 1 << 20


if __name__ == "__main__":
    main()
