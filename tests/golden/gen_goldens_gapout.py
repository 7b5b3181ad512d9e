#!/usr/bin/env python3
"""Golden vectors for the gap filler's output: the reference's own print_gap_filled_sequences (bin/ntlink_patch_gaps.py:533-598, which
prints the filling summary, :668-678) and print_agp (:600-665), nothing wrapped, over the `pairs`, `mappings`, ScaffoldGaps and reads
constructed below -- once without and once with --soft_mask -- and the reference's main() (:760-836) once over its own gap-fill test
(tests/ntlink_pytest.py test_5: scaffolds_1.fa, long_reads_1.fa, -k 35 -w 10 --large_k 32 --min_gap 1), whose FASTA must be the file the
reference ships; its .agp and its summary are recorded.  Output: tests/golden/gen/gapout_cases.json.gz (data only).

Same import recipe and the same `btllib` / `igraph` stubs as gen_goldens_gapmask.py, plus a SeqReader; NTLINK_REFERENCE names the
reference's checkout.  The conditions at the end of main() are what tests/test_gapfill_output.py relies on; if a case misses one,
change the case, not the condition."""
import argparse
import contextlib
import gzip
import io
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

if "NTLINK_REFERENCE" not in os.environ:
    raise SystemExit("NTLINK_REFERENCE must name the reference's checkout")
REFERENCE = os.environ["NTLINK_REFERENCE"]
OUT = os.path.join(REPO, "tests", "golden", "gen", "gapout_cases.json.gz")
ACGT = np.frombuffer(b"ACGT", np.uint8)
MIN_GAP = 20


# ---------------------------------------------------------------- the btllib stub (as in gen_goldens_gapmask.py, and a SeqReader)

class _Mx:
    def __init__(self, h, p, s):
        self.out_hash, self.pos, self.forward = int(h), int(p), bool(s)


class _Record:
    def __init__(self, num, name, seq, k, w):
        self.num, self.id, self.readlen = num, name, len(seq)
        self.minimizers = [_Mx(h, p, s) for h, p, s in zip(*oracle.sketch_seq(seq, k, w))]


class _Reader:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def __iter__(self):
        return self._it

    def read(self):
        return next(self._it)


class _Indexlr(_Reader):
    def __init__(self, path, k, w, flags=0, threads=1):
        self._it = (_Record(i, name, seq, k, w) for i, (name, seq) in enumerate(oracle.read_fastx(path)))


class _SeqReader(_Reader):
    def __init__(self, path, flags=0, threads=1):
        self._it = (types.SimpleNamespace(id=name, seq=seq.decode()) for name, seq in oracle.read_fastx(path))


btllib = types.ModuleType("btllib")
btllib.Indexlr, btllib.SeqReader = _Indexlr, _SeqReader
btllib.IndexlrFlag = types.SimpleNamespace(LONG_MODE=0)
btllib.SeqReaderFlag = types.SimpleNamespace(LONG_MODE=0)
sys.modules["btllib"] = btllib
sys.modules["igraph"] = types.ModuleType("igraph")
sys.path.insert(0, os.path.join(REFERENCE, "bin"))
import ntlink_patch_gaps  # noqa: E402  (the reference)


# ---------------------------------------------------------------- the crafted case

def rand(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes().decode()


PATH = ("ntLink_0\tA+ 50N B- 1N C- 1N D+ 5N E+ 100N F- 30N G+\n"
        "ntLink_1\tH- 200N I+ 60N J- 40N K+ 0N L+\n"
        "a_line_without_a_tab\n"
        "ntLink_2\tM+ 70N N+ 80N O- 90N P-\n"
        "\n"
        "ntLink_3\tQ+\n")


def build(seed=3):
    rng = np.random.default_rng(seed)
    scaffolds, reads = {}, {}
    for name, n in zip("ABCDEFGHIJKLMNOPQ", (120, 95, 131, 60, 77, 150, 88, 140, 200, 111, 90, 64, 105, 99, 123, 81, 70)):
        scaffolds[name] = rand(rng, n)
    scaffolds["B"] = scaffolds["B"][:30] + scaffolds["B"][30:50].lower() + "RYN" + scaffolds["B"][53:]
    scaffolds["C"] = scaffolds["C"][:-1] + "G"              # its reverse complement begins with C: lower-cased behind the 1N join
    scaffolds["E"] = "T" + scaffolds["E"][1:]                # upper case: stays so behind the eroded D
    scaffolds["U1"] = "acgtnnNNRYKM" + rand(rng, 40) + rand(rng, 20).lower() + "swBDHVu"  # in no path
    scaffolds["U2"] = rand(rng, 55)
    for rid, n in (("r_fg", 260), ("r_hi", 180), ("r_ij", 190), ("r_jk", 240), ("r_mn", 210), ("r_no", 230), ("r_op", 170), ("r_ab", 200)):
        reads[rid] = rand(rng, n)
    reads["r_fg"] = reads["r_fg"][:100] + "acgtRYkmN" + reads["r_fg"][109:]
    #           source target gap  read   src_ctg src_read tgt_ctg tgt_read old_anchor  read's orientation on the source
    pairs = [("A+", "B-", 49, "r_ab", 100, 20, 80, 150, False, "+"),     # (+, -), forward
             ("E+", "F-", 99, None, None, None, None, None, False, None),  # no read chosen: the cuts are None
             ("F-", "G+", 29, "r_fg", 10, 190, 15, 60, False, "+"),        # (-, +): the read lies the other way round on F-
             ("H-", "I+", 199, "r_hi", 12, 40, 30, 40, True, "-"),         # equal read cuts: filled with nothing
             ("I+", "J-", 59, "r_ij", 170, 80, 100, 50, False, "+"),       # crossed read cuts, forward: nothing
             ("J-", "K+", 39, "r_jk", 9, 30, 7, 200, True, "-"),           # forward, the old anchors
             ("M+", "N+", 69, "r_mn", 90, 200, 10, 12, False, "-"),        # (+, +), reversed: [12, 200)
             ("N+", "O-", 79, "r_no", 85, 100, 110, 100000, False, "+"),   # a cut beyond the read: the slice ends with the read
             ("O-", "P-", 89, "r_op", 20, 169, 70, 170, False, "-")]       # (-, -), forward, one base
    #            five_prime_cut three_prime_cut five_prime_trim three_prime_trim
    state = {"A": (0, 100, 0, 120), "B": (0, 80, 4, 95), "D": (40, 30, 0, 60),                # D: fully eroded
             "F": (10, 150, 0, 150), "G": (15, 88, 0, 88), "H": (12, 140, 0, 133),
             "I": (30, 170, 41, 200),                                                            # the trim tighter at 5', looser at 3'
             "J": (9, 100, 0, 111), "K": (7, 90, 0, 90), "M": (0, 90, 0, 105), "N": (10, 85, 0, 99), "O": (20, 110, 0, 123),
             "P": (0, 500, 0, 1000),                                                             # a cut and a trim beyond the scaffold
             "U1": (0, len(scaffolds["U1"]), 5, 70)}                                             # unassigned, and trimmed
    return scaffolds, reads, pairs, state


def run_reference(scaffolds, reads, pairs, state, soft_mask):
    """the FASTA, the AGP and the summary the reference's two functions write"""
    scaf = {name: ntlink_patch_gaps.ScaffoldGaps(seq) for name, seq in scaffolds.items()}
    for name, (c5, c3, t5, t3) in state.items():
        scaf[name].five_prime_cut, scaf[name].three_prime_cut, scaf[name].five_prime_trim, scaf[name].three_prime_trim = c5, c3, t5, t3
    info, mappings = {}, {}
    for source, target, gap, read, sc, sr, tc, tr, old, ori in pairs:
        p = ntlink_patch_gaps.PairInfo(gap)
        p.chosen_read, p.source_ctg_cut, p.source_read_cut, p.target_ctg_cut, p.target_read_cut, p.old_anchor_used = read, sc, sr, tc, tr, old
        info[(source, target)] = p
        if read is not None:
            mappings.setdefault(read, {})[source.strip("+-")] = types.SimpleNamespace(orientation=ori)
    with tempfile.TemporaryDirectory() as tmp:
        path_file = os.path.join(tmp, "c.path")
        with open(path_file, "w") as fh:
            fh.write(PATH)
        args = argparse.Namespace(o=os.path.join(tmp, "c.fa"), path=path_file, min_gap=MIN_GAP + 1, soft_mask=soft_mask, verbose=False)
        stats = io.StringIO()
        with contextlib.redirect_stdout(stats):
            ntlink_patch_gaps.print_gap_filled_sequences(info, mappings, scaf, reads, args)
        ntlink_patch_gaps.print_agp(info, mappings, scaf, args)
        return {"fasta": open(args.o).read(), "agp": open(args.o + ".agp").read(), "stats": stats.getvalue()}


def run_shipped():
    """the reference's main() over its own gap-fill test: (.agp, summary), the FASTA compared with the shipped file"""
    data = os.path.join(REFERENCE, "tests")
    prefix = os.path.join(data, "expected_outputs", "scaffolds_1.fa.k32.w250.z1000.")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.gap_fill.fa")
        argv = ["ntlink_patch_gaps.py", "--path", prefix + "trimmed_scafs.path", "--mappings", prefix + "verbose_mapping.tsv", "--trims",
                prefix + "trimmed_scafs.tsv", "-s", os.path.join(data, "scaffolds_1.fa"), "--reads", os.path.join(data, "long_reads_1.fa"),
                "--large_k", "32", "--min_gap", "1", "-k", "35", "-w", "10", "-o", out]
        log, saved = io.StringIO(), sys.argv
        sys.argv = argv
        try:
            with contextlib.redirect_stdout(log):
                ntlink_patch_gaps.main()
        finally:
            sys.argv = saved
        assert open(out, "rb").read() == open(prefix + "ntLink.scaffolds.gap_fill.fa", "rb").read(), "the reference's shipped golden"
        text = log.getvalue()
        at = text.index("\nGap filling summary:")
        stats = text[at:text.index("\n\n", at + 1) + 2]
        return open(out + ".agp").read(), stats


def main():
    scaffolds, reads, pairs, state = build()
    plain = run_reference(scaffolds, reads, pairs, state, False)
    soft = run_reference(scaffolds, reads, pairs, state, True)
    records = dict(zip(*[iter(plain["fasta"].split("\n")[:-1])] * 2))
    agp = [row.split("\t") for row in plain["agp"].splitlines()]
    in_pairs = {(p[0], p[1]) for p in pairs}
    rc = ntlink_patch_gaps.ScaffoldGaps.reverse_complement
    line0 = records[">ntLink_0"]
    # a 1N join followed by a `-` node: the first base of C's reverse complement is lower-cased

    def cut(name):
        c5, c3, t5, t3 = state.get(name, (0, len(scaffolds[name]), 0, len(scaffolds[name])))
        return scaffolds[name][max(c5, t5):min(c3, t3)]

    c_piece = rc(cut("C"))
    assert c_piece[0] == "C" and "c" + c_piece[1:] in line0 and c_piece not in line0
    # a 1N join followed by a fully eroded scaffold: nothing of D, and E keeps its upper-case first base
    assert cut("D") == "" and ("c" + c_piece[1:] + "NNNN" + cut("E")) in line0 and cut("E")[0] == "T"
    assert not any(row[5] == "D" for row in agp)
    # a small gap that is not in pairs: four N in the FASTA, a row that does not advance the component number
    assert ("D+", "E+") not in in_pairs
    n_row = next(i for i, row in enumerate(agp) if row[0] == "ntLink_0" and row[4] == "N" and row[5] == "4")
    assert agp[n_row + 1][3] == agp[n_row][3]
    # None cuts
    assert "N" * 99 in line0 and any(row[4] == "N" and row[5] == "99" for row in agp)
    # a reversed read without and with soft_mask; lower case and IUPAC codes of the read survive
    fg = rc(reads["r_fg"][60:190])
    assert fg in line0 and fg.lower() in dict(zip(*[iter(soft["fasta"].split("\n")[:-1])] * 2))[">ntLink_0"] and fg != fg.lower() != fg.upper()
    assert plain["agp"] == soft["agp"] and plain["stats"] == soft["stats"] and plain["fasta"] != soft["fasta"]
    # equal read cuts and crossed read cuts: counted as filled, nothing written, no row
    assert not any(row[5] in ("r_hi", "r_ij") for row in agp)
    line1 = records[">ntLink_1"]
    assert line1.startswith(rc(cut("H")) + cut("I") + rc(cut("J")))
    # trims tighter than the cut at one end and looser at the other; a scaffold that is the target of one gap and the source of the next
    assert state["I"][2] > state["I"][0] and state["I"][3] > state["I"][1] and cut("I") == scaffolds["I"][41:170]
    assert ("H-", "I+") in in_pairs and ("I+", "J-") in in_pairs
    # 0N: nothing in either file
    assert (cut("K") + cut("L")) in line1
    # all four sign pairs among the pairs with a read; a cut beyond the read
    assert {(p[0][-1], p[1][-1]) for p in pairs if p[3]} == {("+", "+"), ("+", "-"), ("-", "+"), ("-", "-")}
    assert reads["r_no"][100:] in records[">ntLink_2"]
    # unassigned scaffolds with lower case and IUPAC codes: whole in the FASTA, the cut coordinates in the AGP
    assert records[">U1"] == scaffolds["U1"] and any(c in scaffolds["U1"] for c in "RYKM") and scaffolds["U1"] != scaffolds["U1"].upper()
    assert [row for row in agp if row[0] == "U1"] == [["U1", "6", "70", "1", "W", "U1", "6", "70", "+"]]
    # a line without a tab, and an empty one
    assert "a_line_without_a_tab" not in plain["fasta"] and list(records) == [">ntLink_0", ">ntLink_1", ">ntLink_2", ">ntLink_3", ">U1", ">U2"]
    shipped_agp, shipped_stats = run_shipped()
    rows = [row.split("\t") for row in shipped_agp.splitlines()]
    assert len(rows) == 3 and [r[4] for r in rows] == ["W", "P", "W"] and rows[0][5:] == ["188266", "1", "33470", "+"]
    assert rows[1][6:] == ["6398", "12089", "+"] and rows[2][5:] == ["189231", "1", "48258", "-"]
    print(plain["stats"], shipped_stats, shipped_agp)
    doc = {"min_gap": MIN_GAP + 1, "path": PATH, "scaffolds": [[n, s] for n, s in scaffolds.items()], "reads": [[i, s] for i, s in reads.items()],
           "pairs": [list(p[:9]) + [p[9] is not None and p[9] != p[0][-1]] for p in pairs], "state": {n: list(v) for n, v in state.items()},
           "plain": plain, "soft_mask": soft, "shipped": {"agp": shipped_agp, "stats": shipped_stats}}
    raw = json.dumps(doc, separators=(",", ":")).encode()
    with open(OUT, "wb") as fh, gzip.GzipFile(filename="", mode="wb", fileobj=fh, mtime=0) as gz:
        gz.write(raw)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) <= 1 << 20


if __name__ == "__main__":
    main()
