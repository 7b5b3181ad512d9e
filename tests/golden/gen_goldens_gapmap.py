#!/usr/bin/env python3
"""Golden vectors for ntlink_amd.gapfill: the reference's own map_long_reads (bin/ntlink_patch_gaps.py:412-442) over synthetic gaps.
Output: tests/golden/gen/gapmap_cases.json.gz (data only).  Same import recipe as tests/golden/gen_goldens.py, with two stubs:
`igraph` (empty, as there) and `btllib` -- a module whose Indexlr yields records made from the oracle's sketch (oracle.sketch_seq) of
the two FASTA files this script writes into a temporary directory.  ntlink_utils.get_accepted_anchor_contigs is wrapped: it records
its arguments and what the reference returns for them, and hands map_long_reads an empty result, so that the loop takes its
`len(accepted_anchor_contigs) != 2` branch (with --stringent: two assignments) and never enters the cut-finding code behind it, which is
outside this fixture.  Everything in front of the call -- the lockstep reading, the header parsing, read_btllib_minimizers, the read's
filtered minimizer list -- is the reference's.

About 64 gaps at k20 w10, mapped once with the default parameters and once with --sensitive.  Pieces are random sequence, flanks
300 .. 3000 bases, reads with 5 % errors, every record N-masked to its full length as print_masked_sequences writes them.  The special
gaps carry their case in the read's name (SPECIAL); the conditions at the end of main() are checked when the file is made."""
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

K, W = 20, 10
OUT = os.path.join(REPO, "tests", "golden", "gen", "gapmap_cases.json.gz")
SPECIAL = ["one_flank", "internal_repeat", "shared_flank_1", "shared_flank_2", "short_scaffold", "read_all_N", "scaffold_all_N", "equal_names"]
ACGT = np.frombuffer(b"ACGT", np.uint8)


# ---------------------------------------------------------------- the btllib stub

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
import ntlink_utils  # noqa: E402


# ---------------------------------------------------------------- the gaps

def rand(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def with_errors(seq, rng, rate=0.05):
    """substitutions, insertions and deletions, a third each"""
    out = bytearray()
    for c in seq:
        r = rng.random()
        if r < rate / 3:
            out.append(ACGT[rng.integers(0, 4)])
        elif r < 2 * rate / 3:
            out.append(c); out.append(ACGT[rng.integers(0, 4)])
        elif r < rate:
            continue
        else:
            out.append(c)
    return bytes(out)


def revcomp(seq):
    return seq.translate(bytes.maketrans(b"ACGTN", b"TGCAN"))[::-1]


def make_gaps(n, seed=7):
    rng = np.random.default_rng(seed)
    scaffolds, reads, tags = [], [], []
    shared = rand(rng, 1500)
    for g in range(n):
        tag = SPECIAL[g // 7] if g % 7 == 3 and g // 7 < len(SPECIAL) else "plain"
        src_flank, tgt_flank = rand(rng, int(rng.integers(300, 3001))), rand(rng, int(rng.integers(300, 3001)))
        src_more, tgt_more = int(rng.integers(0, 3000)), int(rng.integers(0, 3000))  # the masked rest of the two scaffolds
        if tag == "internal_repeat":
            src_flank = src_flank[:900] + src_flank[300:700] + src_flank[900:]  # 400 bases twice: their minimizers drop out of the gap's dict
        if tag.startswith("shared_flank"):
            src_flank = shared  # the same flank, verbatim, in two gaps: the same hashes in two groups
        if tag == "short_scaffold":
            tgt_flank, tgt_more = tgt_flank[:600], 200  # 800 bases in all: shorter than z
            src_more += 1000
        reach_s, reach_t = int(rng.integers(250, 900)), int(rng.integers(250, 900))
        if tag == "one_flank":
            reach_t = 0
        piece = src_flank[-reach_s:] + rand(rng, int(rng.integers(50, 400))) + (tgt_flank[:reach_t] if reach_t else b"")
        piece = with_errors(piece, rng)
        before, after = int(rng.integers(0, 2000)), int(rng.integers(0, 2000))
        read = b"N" * before + piece + b"N" * after
        if tag == "read_all_N":
            read = b"N" * len(read)
        if rng.random() < 0.3:
            read = revcomp(read)
        src = b"N" * src_more + src_flank
        tgt = tgt_flank + b"N" * tgt_more
        if tag == "scaffold_all_N":
            tgt = b"N" * len(tgt)
        sname, tname = f"scaf{2 * g}{'+-'[g % 2]}", f"scaf{2 * g + 1}{'+-'[(g // 2) % 2]}"
        if tag == "equal_names":  # the two ends of ONE scaffold, in both orientations: one name after the signs are stripped
            sname, tname = f"scaf{2 * g}+", f"scaf{2 * g}-"
            total = max(len(src), len(tgt))
            src, tgt = b"N" * (total - len(src_flank)) + src_flank, tgt_flank + b"N" * (total - len(tgt_flank))
        scaffolds += [(sname + "_source", src), (tname + "_target", tgt)]
        reads.append((f"{tag}-{g}__{sname}__{tname}", read))
        tags.append(tag)
    return scaffolds, reads, tags


def run_reference(scaffolds, reads, sensitive):
    """the reference's map_long_reads over the two files; [(order, {contig: hits})] per gap"""
    calls = []
    real = ntlink_utils.get_accepted_anchor_contigs

    def recording(mx_list, read_length, scaf, mx_info, args):
        accepted, order = real(mx_list, read_length, scaf, mx_info, args)
        calls.append((list(order), {c: [[h.mx, h.ctg_pos, h.ctg_strand, h.read_pos, h.read_strand] for h in run.hits]
                                              for c, run in accepted.items()}))
        return {}, order

    by_name = {}
    for sid, seq in scaffolds:
        name = sid.rsplit("_", 1)[0].strip("+-")
        assert by_name.setdefault(name, len(seq)) == len(seq)
    scaf = {name: ntlink_utils.Scaffold(id=name, length=length) for name, length in by_name.items()}
    pairs = {tuple(rid.split("__")[1:]): types.SimpleNamespace(source_read_cut=0, target_read_cut=0) for rid, _seq in reads}
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "g")
        for path, recs in ((prefix + ".scaffolds.masked_temp.fa", scaffolds), (prefix + ".reads.masked_temp.fa", reads)):
            with open(path, "wb") as fh:
                for rid, seq in recs:
                    fh.write(b">" + rid.encode() + b"\n" + seq + b"\n")
        args = argparse.Namespace(o=prefix, k=K, w=W, t=1, z=1000, x=0.0, sensitive=sensitive, stringent=True)
        ntlink_utils.get_accepted_anchor_contigs = recording
        try:
            ntlink_patch_gaps.map_long_reads(pairs, scaf, args)
        finally:
            ntlink_utils.get_accepted_anchor_contigs = real
    assert len(calls) == len(reads)
    return calls, {"k": K, "z": 1000, "x": 0.0, "sensitive": sensitive}


def main():
    scaffolds, reads, tags = make_gaps(64)
    sets = []
    for sensitive in (False, True):
        calls, params = run_reference(scaffolds, reads, sensitive)
        sets.append({"params": params, "gaps": [{"order": order, "hits": hits} for order, hits in calls]})
        two = sum(1 for order, _ in calls if len(order) == 2)
        assert 2 * two >= len(calls), f"only {two} of {len(calls)} gaps have exactly two accepted contigs"
        print(f"sensitive={sensitive}: {two} of {len(calls)} gaps with two accepted contigs")
    assert all(t in tags for t in SPECIAL), "every special case is present by name"
    first = {t: tags.index(t) for t in SPECIAL}
    gaps = sets[0]["gaps"]
    assert len(gaps[first["one_flank"]]["order"]) != 2 and len(gaps[first["read_all_N"]]["order"]) == 0
    assert len(gaps[first["scaffold_all_N"]]["order"]) < 2 and len(gaps[first["short_scaffold"]]["order"]) < 2
    assert len(gaps[first["equal_names"]]["order"]) <= 1
    assert len(gaps[first["shared_flank_1"]]["order"]) == 2 and len(gaps[first["shared_flank_2"]]["order"]) == 2
    doc = {"k": K, "w": W, "tags": tags, "scaffolds": [[i, s.decode()] for i, s in scaffolds], "reads": [[i, s.decode()] for i, s in reads],
           "sets": sets}
    raw = json.dumps(doc, separators=(",", ":")).encode()
    with open(OUT, "wb") as fh, gzip.GzipFile(filename="", mode="wb", fileobj=fh, mtime=0) as gz:
        gz.write(raw)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) <= 1 << 20


if __name__ == "__main__":
    main()
