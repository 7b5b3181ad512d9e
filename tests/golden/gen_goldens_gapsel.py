#!/usr/bin/env python3
"""Golden vectors for ntlink_amd.gapfill.choose_gap_reads: the reference's own read_path_file_pairs, read_verbose_mappings,
choose_best_read_per_pair and find_masking_cut_points (bin/ntlink_patch_gaps.py:94-111, 178-198, 249-261, 311-342), nothing wrapped, over
a verbose file made of tests/golden/gen/fixtures/t3_k24_w250.verbose_mapping.tsv (the path file joins the contigs its reads map to in a
row) and the reads crafted below for the branches those do not reach.  Output: tests/golden/gen/gapsel_cases.json.gz (data only): the
inputs -- verbose text, path text, contig lengths, large_k, min_gap -- and per pair sorted(mapping_reads), chosen_read and the four
cuts.

Same import recipe and the same `btllib` / `igraph` stubs as gen_goldens_gapcuts.py (nothing of btllib is called here).  The conditions
at the end of main() say which branch every crafted pair takes; if a crafted read misses its branch, change the read, not the
condition."""
import argparse
import gzip
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BASE = os.path.join(REPO, "tests", "golden", "gen", "fixtures", "t3_k24_w250.verbose_mapping.tsv")
OUT = os.path.join(REPO, "tests", "golden", "gen", "gapsel_cases.json.gz")
LARGE_K, MIN_GAP, LEN = 24, 20, 10000

sys.modules["btllib"] = types.ModuleType("btllib")
sys.modules["igraph"] = types.ModuleType("igraph")
sys.path.insert(0, os.environ.get("NTLINK_REFERENCE_BIN", "/root/reference/bin"))
import ntlink_patch_gaps  # noqa: E402  (the reference)
import ntlink_utils  # noqa: E402

FLIP = {"+": "-", "-": "+"}


# ---------------------------------------------------------------- the crafted reads

def run(n, cpos, cstep, rpos, ori, rstep=40, rstrand="+"):
    """n hits from (cpos, rpos) on: contig positions in steps of cstep, the read's strand rstrand, the contig's by the orientation"""
    cstrand = rstrand if ori == "+" else FLIP[rstrand]
    return [(cpos + i * cstep, cstrand, rpos + i * rstep, rstrand) for i in range(n)]


def line(read, ctg, anchors, hits):
    return f"{read}\t{ctg}\t{anchors}\t" + " ".join(f"{c}:{cs}_{r}:{rs}" for c, cs, r, rs in hits)


def near(sign_is_ori_plus, source):
    """where on a contig of LEN a mapping of 5 hits lies so that the distance to the gap is small: a source in '+' ends near the
    contig's end, in '-' near its start (calculate_est_gap_size, :212-219); a target the other way round.  -> (cpos, cstep)"""
    at_end = sign_is_ori_plus == source
    if at_end:
        return (LEN - 400, 50) if source else (LEN - 200, -50)  # the terminal hit (source: last, target: first) is the one nearest the end
    return (300, -50) if source else (100, 50)


def support(read, src, s_ori, tgt, t_ori, anchors=(5, 5), rpos=1000, n=5, gap=300):
    """two lines: `read` maps src with orientation s_ori, then tgt with t_ori, each with n hits near the gap between them"""
    c0, step = near(s_ori == "+", True)
    first = run(n, c0, step, rpos, s_ori)
    c1, step = near(t_ori == "+", False)
    second = run(n, c1, step, first[-1][2] + gap, t_ori)
    return [line(read, src, anchors[0], first), line(read, tgt, anchors[1], second)]


def crafted():
    """(verbose lines, path lines, tags: pair -> what it is there for)"""
    v, p, tags = [], [], {}

    def path(tag, src, tgt, gap=500):
        p.append(f"{tag}\t{src} {gap}N {tgt}")
        tags[tag] = (src, tgt)

    # support through the reverse complement: the read meets x2 then x1, both against the path's signs
    path("revcomp", "x1+", "x2+")
    v += support("rc_read", "x2", "-", "x1", "-")
    # a mapping with mixed strands / with non-monotone positions is skipped: the pair gets no read
    path("mixed", "m1+", "m2+")
    lines = support("mixed_read", "m1", "+", "m2", "+")
    f = lines[1].split("\t")
    toks = f[3].split(" ")
    toks[2] = toks[2].replace(":+_", ":-_")
    v += [lines[0], "\t".join(f[:3] + [" ".join(toks)])]
    path("positions", "n1+", "n2+")
    lines = support("positions_read", "n1", "+", "n2", "+")
    f = lines[1].split("\t")
    toks = f[3].split(" ")
    toks[1], toks[2] = toks[2], toks[1]
    v += [lines[0], "\t".join(f[:3] + [" ".join(toks)])]
    # `length` from an earlier mapping because the last one is invalid: with the junk line's read positions the estimate would pass
    path("length", "p1+", "p2+")
    v += [line("length_read", "p1", 5, run(5, 1000, 50, 1000, "+")), line("length_read", "p2", 5, run(5, 100, 50, 1500, "+")),
          line("length_read", "p3", 5, [(10, "+", 30000, "+"), (20, "-", 30100, "+")])]
    # three mappings whose non-adjacent combination is a pair
    path("skip_one", "q1+", "q3+")
    lines = support("skip_read", "q1", "+", "q3", "+", gap=900)
    v += [lines[0], line("skip_read", "q2", 7, run(3, 5000, 50, 1300, "-")), lines[1]]
    # a path holding (i, j) and its reverse complement as separate pairs: one read supports both
    path("both_fwd", "r1+", "r2+")
    path("both_rev", "r2-", "r1-")
    v += support("both_read", "r1", "+", "r2", "+")
    # a gap <= min_gap is left out
    path("small_gap", "s1+", "s2+", gap=MIN_GAP)
    v += support("small_read", "s1", "+", "s2", "+")
    # equal anchor sums decided by the name as a string: read9 > read10
    path("by_name", "t1+", "t2+")
    v += support("read10", "t1", "+", "t2", "+", anchors=(4, 6)) + support("read9", "t1", "+", "t2", "+", anchors=(5, 5), rpos=2000)
    # the best read invalid by its gap estimate (far from the contig's end), the second taken
    path("second", "u1+", "u2+")
    v += [line("u_best", "u1", 20, run(5, 1000, 50, 1000, "+")), line("u_best", "u2", 20, run(5, 100, 50, 1500, "+"))]
    v += support("u_second", "u1", "+", "u2", "+")
    # every read invalid
    path("none_valid", "v1+", "v2+")
    v += [line("v_far", "v1", 9, run(5, 1000, 50, 1000, "+")), line("v_far", "v2", 9, run(5, 100, 50, 1500, "+"))]
    # single-hit mappings: one hit is every orientation's and every order's
    path("single", "w1+", "w2-")
    v += support("single_read", "w1", "+", "w2", "-", n=1)
    # situations A-D (:276-288) on either side: every pair of signs, supported directly and through the reverse complement
    for n, (ss, ts) in enumerate(("++", "+-", "-+", "--")):
        path(f"direct{ss}{ts}", f"d{n}a{ss}", f"d{n}b{ts}")
        v += support(f"direct_read{n}", f"d{n}a", ss, f"d{n}b", ts)
        path(f"via{ss}{ts}", f"e{n}a{ss}", f"e{n}b{ts}")
        v += support(f"via_read{n}", f"e{n}b", FLIP[ts], f"e{n}a", FLIP[ss])
    return v, p, tags


# ---------------------------------------------------------------- the fixture's own reads

def base_paths(text):
    """the contigs a read of the fixture maps to in a row, joined in a path: every second one as its reverse complement"""
    paths, lengths, rows = [], {}, {}
    for row in text.splitlines():
        read, ctg, _n, mxs = row.split("\t")
        mxs = ntlink_utils.parse_minimizers(mxs)
        lengths[ctg] = max(lengths.get(ctg, 0), max(m.ctg_pos for m in mxs) + LARGE_K + 100)
        ori = ntlink_patch_gaps.find_orientation(mxs)
        if ori is not None and ntlink_patch_gaps.check_position_consistency(mxs):
            rows.setdefault(read, []).append(ctg + ori)
    seen = set()
    for read, order in rows.items():
        for i, j in zip(order, order[1:]):
            if len(paths) % 2:
                i, j = ntlink_patch_gaps.reverse_complement_pair(i, j)
            if (i, j) not in seen and ntlink_patch_gaps.reverse_complement_pair(i, j) not in seen and i[:-1] != j[:-1]:
                seen.add((i, j))
                paths.append(f"base{len(paths)}\t{i} 1000N {j}")
    return paths, lengths


def main():
    with open(BASE) as fh:
        base = fh.read()
    paths, lengths = base_paths(base)
    assert len(paths) >= 5, paths
    more_v, more_p, tags = crafted()
    verbose = base + "".join(row + "\n" for row in more_v)
    path_text = "".join(row + "\n" for row in paths + more_p)
    for row in more_v:
        lengths.setdefault(row.split("\t")[1], LEN)
    sequences = {name: types.SimpleNamespace(length=length) for name, length in lengths.items()}
    args = argparse.Namespace(large_k=LARGE_K)
    with tempfile.TemporaryDirectory() as tmp:
        vp, pp = os.path.join(tmp, "g.verbose_mapping.tsv"), os.path.join(tmp, "g.path")
        with open(vp, "w") as fh:
            fh.write(verbose)
        with open(pp, "w") as fh:
            fh.write(path_text)
        pairs = ntlink_patch_gaps.read_path_file_pairs(pp, MIN_GAP)
        mappings = ntlink_patch_gaps.read_verbose_mappings(vp, pairs)
        ntlink_patch_gaps.choose_best_read_per_pair(pairs, mappings, sequences, args)
        ntlink_patch_gaps.find_masking_cut_points(pairs, mappings, args)
    state = {f"{s} {t}": [sorted(p.mapping_reads), p.chosen_read, p.source_ctg_cut, p.source_read_cut, p.target_ctg_cut, p.target_read_cut]
             for (s, t), p in pairs.items()}
    at = {tag: state.get(f"{s} {t}") for tag, (s, t) in tags.items()}
    base_ctgs = {row.split("\t")[1] for row in base.splitlines()}
    n_base = sum(1 for key, got in state.items() if key.split(" ")[0][:-1] in base_ctgs and got[1] is not None)
    print(f"{len(pairs)} pairs, {sum(1 for g in state.values() if g[1] is not None)} with a chosen read, {n_base} of them from the fixture's reads")
    assert n_base >= 3
    assert at["revcomp"][1] == "rc_read"
    assert at["mixed"][:2] == [[], None] and at["positions"][:2] == [[], None]
    assert at["length"][:2] == [["length_read"], None] and mappings["length_read"]["length"] < 2000
    assert at["skip_one"][1] == "skip_read"
    assert at["both_fwd"][1] == "both_read" and at["both_rev"][1] == "both_read" and at["both_fwd"][2:] != at["both_rev"][2:]
    assert at["small_gap"] is None and "small_read" not in mappings
    assert at["by_name"][:2] == [["read10", "read9"], "read9"]
    assert at["second"][:2] == [["u_best", "u_second"], "u_second"]
    assert at["none_valid"][:2] == [["v_far"], None]
    assert at["single"][1] == "single_read"
    for side in (0, 1):  # (the contig's sign, the read-based orientation) of the chosen reads, for a source and for a target
        got = {(key.split(" ")[side][-1], mappings[g[1]][key.split(" ")[side][:-1]].orientation) for key, g in state.items() if g[1] is not None}
        assert got == {("+", "+"), ("+", "-"), ("-", "-"), ("-", "+")}, (side, got)
    for tag, got in at.items():
        if tag.startswith(("direct", "via")):
            assert got[1] is not None and None not in got[2:], (tag, got)
    doc = {"large_k": LARGE_K, "min_gap": MIN_GAP, "verbose": verbose, "path": path_text, "lengths": lengths,
           "tags": {tag: f"{s} {t}" for tag, (s, t) in tags.items()}, "pairs": state}
    raw = json.dumps(doc, separators=(",", ":")).encode()
    with open(OUT, "wb") as fh, gzip.GzipFile(filename="", mode="wb", fileobj=fh, mtime=0) as gz:
        gz.write(raw)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) <= 1 << 20


if __name__ == "__main__":
    main()
