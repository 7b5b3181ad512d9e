"""The merge stage on the host (ntlink_amd/merge.py: merge_plan, fac_stats), no device: the plan rendered in plain Python.
  a. the reference's four cases byte for byte (tests/golden/ref/expected_outputs: .trimmed_scafs.fa.gz + .trimmed_scafs.path ->
     .stitch.abyss-scaffold.fa.gz), and their abyss-fac lines from the called bases of that file -- all four fit "ACGT of either case"
  b. crafted paths of 1, 3, 5 and 7 nodes: headers, LEN, COMMENT, segments; 1N, 2N, `-` and `+` mixed; an unpathed contig whose
     header has a comment; a contig that is a lone N behind a join; lines without a tab.  Contigs and gaps must alternate, so paths
     of 2 and 4 nodes are among the refusals
  c. every refusal, with the line and the node in the message
  d. fac_stats: a record below 500 dropped from n:500; none left; ties and the weighted percentiles"""
import numpy as np
import pytest

import merge_cases as mc
from ntlink_amd import capi, merge

FILL, REV, FIRST = capi.NTL_STITCH_FILL, capi.NTL_STITCH_REVCOMP, capi.NTL_STITCH_LOWER_FIRST


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_reference_case(n):
    recs = mc.read_fasta(mc.trimmed_fasta(n))
    assert merge.fasta_headers(mc.trimmed_fasta(n)) == [h for h, _s in recs]
    contigs = merge.Contigs.whole([h.split()[0].decode() for h, _s in recs], [len(s) for _h, s in recs], [h for h, _s in recs])
    plan = merge.merge_plan(mc.case_file(n, ".trimmed_scafs.path"), contigs)
    assert plan.n_unpathed == 0
    assert mc.render(plan, [s for _h, s in recs]) == mc.golden(n)
    with open(mc.case_file(n, ".ntLink.scaffolds.fa.abyssfac.tsv")) as fh:
        want = fh.read()
    assert merge.fac_text(merge.fac_stats(mc.counts_of_fasta(mc.golden(n))), mc.CASES[n] + ".ntLink.scaffolds.fa") == want


def test_case_1_counting_rule():
    "87401 bytes, 4541 N and one n that the input carries through: 82859 called bases"
    seq = mc.golden(1).split(b"\n")[1]
    assert (len(seq), seq.count(b"N"), seq.count(b"n")) == (87401, 4541, 1)
    assert mc.counts_of_fasta(mc.golden(1)).tolist() == [82859]


SEQS = {"a": b"ACGTNacgtn", "b": b"GGGTTTCA", "c": b"T", "d": b"RYKMacgu", "e": b"CCCCCCCCCCCC", "f": b"AGAGAGA", "g": b"TTTTG", "h": b"ACCA",
        "i": b"GATTACA", "j": b"CAT", "free1": b"ACGTAC", "free2": b"nnNN"}
HEADERS = {"free1": b"free1 12-7 some comment", "free2": b"free2"}


def crafted(tmp_path, lines, seqs=SEQS):
    path = tmp_path / "x.path"
    path.write_text("".join(line + "\n" for line in lines))
    ids = list(seqs)
    contigs = merge.Contigs.whole(ids, [len(seqs[i]) for i in ids], [HEADERS.get(i, i.encode()) for i in ids])
    return merge.merge_plan(str(path), contigs), [seqs[i] for i in ids]


def rc(seq):
    return seq[::-1].translate(mc.TABLE)


def test_crafted_paths(tmp_path):
    lines = ["p1\tc+",                                         # one node
             "this line has no tab",
             "p2\ta+ 5N b-",                                   # three nodes
             "",
             "p4\td- 1N e+ 2N f- 11N g+",                      # seven nodes: first,...,last
             "p3\th+ 1N i-",                                   # 1N: nothing between, the next contig's first base lower-cased
             "p5\tj- 3N free2+"]
    plan, seqs = crafted(tmp_path, lines)
    S = SEQS
    want = [b">free1 12-7 some comment\n" + S["free1"] + b"\n",
            b">p1 1 0 c+\nT\n",
            b">p2 22 0 a+,5N,b-\n" + S["a"] + b"NNNN" + rc(S["b"]) + b"\n",
            b">p4 43 0 d-,...,g+\n" + rc(S["d"]) + b"c" + S["e"][1:] + b"N" + rc(S["f"]) + b"N" * 10 + S["g"] + b"\n",
            b">p3 11 0 h+,1N,i-\n" + S["h"] + b"t" + rc(S["i"])[1:] + b"\n",
            b">p5 9 0 j-,3N,free2+\n" + rc(S["j"]) + b"NN" + S["free2"] + b"\n"]
    assert rc(S["d"]) == b"acgtKMRY" and rc(S["i"]) == b"TGTAATC"
    assert mc.render(plan, seqs) == b"".join(want)
    assert plan.n_unpathed == 1 and plan.seq_len.tolist() == [6, 1, 22, 43, 11, 9]
    assert plan.headers == [w.split(b"\n")[0] + b"\n" for w in want]
    ids = list(SEQS)
    recs = list(plan.records())
    assert recs[2][1] == [(0, ids.index("a"), 0, 10, 0), (FILL, ord("N"), 0, 4, 0), (0, ids.index("b"), 0, 8, REV)]
    assert recs[4][1] == [(0, ids.index("h"), 0, 4, 0), (0, ids.index("i"), 0, 7, REV | FIRST)]  # the 1N gap is no segment
    assert [size for _h, _s, size in recs] == [len(w) for w in want]


def test_comment_boundary_at_four_nodes(tmp_path):
    """up to 3 nodes joined, more `first,...,last`.  Contigs and gaps alternate in every path that is not refused, so a path has 1, 3,
    5, ... nodes: the 2- and 4-node paths are refusals (test_refusals), and 3 and 5 are the two sides of ABySS's boundary at 4"""
    seqs = {name: b"ACGT" for name in "abcde"}
    path = tmp_path / "y.path"
    contigs = merge.Contigs.whole(list(seqs), [4] * 5)
    for nodes, comment in (("a+ 2N b+", "a+,2N,b+"), ("a+ 2N b+ 2N c-", "a+,...,c-"), ("a+ 2N b+ 2N c- 9N d+ 1N e-", "a+,...,e-")):
        path.write_text(f"s\t{nodes}\n")
        plan = merge.merge_plan(str(path), contigs)
        assert plan.headers[-1].split(b" ")[-1] == comment.encode() + b"\n"


def test_trimmed_forms(tmp_path):
    "contigs as slices of larger records, and a contig that is a lone N, behind a gap and behind a join (trimmed_contigs' forms)"
    store = [b"ttACGTACGTgg", b"", b"CCCAAAT"]
    contigs = merge.Contigs(["x", "n", "y", "z"], [0, -1, 2, -1], [2, 0, 1, 0], [10, 1, 6, 1], [b"x 2-10", b"n None-None", b"y 1-6", b"z 0-0"])
    path = tmp_path / "t.path"
    path.write_text("s\tx- 1N n+ 4N y+\n")
    plan = merge.merge_plan(str(path), contigs)
    assert mc.render(plan, store) == b">z 0-0\nN\n>s 17 0 x-,...,y+\nACGTACGTnNNNCCAAA\n"
    assert list(plan.records())[1][1] == [(0, 0, 2, 10, REV), (FILL, ord("n"), 0, 1, 0), (FILL, ord("N"), 0, 3, 0), (0, 2, 1, 6, 0)]


@pytest.mark.parametrize("line, node, why", [
    ("p\ta+ 5N nosuch-", "nosuch-", "no contig nosuch"),
    ("p\ta+ 5N b- 7N a-", "a-", "already used"),
    ("p\ta+ b-", "b-", "no gap between"),           # 2 nodes
    ("p\ta+ 2N b+ c+", "c+", "no gap between"),     # 4 nodes
    ("p\ta+ b+ 2N c+", "b+", "no gap between"),
    ("p\t5N a+", "5N", "end of a path"),
    ("p\ta+ 5N", "5N", "end of a path"),
    ("p\ta+ 0N b+", "0N", "0N"),
    ("p\ta+ 3N 4N b+", "4N", "two gaps"),
    ("p\ta+ 5N b", "b", "must end in"),
    ("p\ta+ 5N b*", "b*", "must end in"),
    ("p\ta+ xN b+", "xN", "must end in"),
    ("p\ta+ 5N +", "+", "must end in"),
])
def test_refusals(tmp_path, line, node, why):
    with pytest.raises(ValueError) as e:
        crafted(tmp_path, ["ok\tc+ 2N d+", line])
    assert f"x.path:2: node {node!r}" in str(e.value) and why in str(e.value)


def test_contig_used_in_two_paths(tmp_path):
    with pytest.raises(ValueError, match=r"x.path:3: node 'a-'.*already used, at line 1"):
        crafted(tmp_path, ["p\ta+ 5N b-", "q\tc+", "r\td+ 2N a-"])


def test_fac_stats():
    keys = ["n", "n:500", "L50", "min", "N75", "N50", "N25", "E-size", "max", "sum"]
    st = merge.fac_stats([499, 500, 1000, 0])
    assert list(st) == keys
    assert list(st.values()) == [4, 2, 1, 500, 500, 1000, 1000, (500 * 500 + 1000 * 1000) // 1500, 1000, 1500]
    assert list(merge.fac_stats([499, 3], min_len=500).values()) == [2] + [0] * 9
    assert list(merge.fac_stats([]).values()) == [0] * 10
    assert list(merge.fac_stats([5, 7], min_len=6)) == ["n", "n:6"] + keys[2:]
    # fixture 3: 86474.95 truncated
    assert merge.fac_stats([82859, 89811])["E-size"] == 86474 and (82859 ** 2 + 89811 ** 2) / 172670 > 86474.9
    # the weighted percentile from the small end: sizes 1000, 2000, 3000 -> half of 6000 is reached at 2000
    st = merge.fac_stats([3000, 1000, 2000])
    assert (st["N75"], st["N50"], st["N25"], st["L50"]) == (2000, 2000, 3000, 2)
    # sums beyond 2^53 stay exact
    big = merge.fac_stats(np.array([3_000_000_001, 3_000_000_003], np.uint64))
    assert big["E-size"] == (3_000_000_001 ** 2 + 3_000_000_003 ** 2) // 6_000_000_004
    assert merge.fac_text(st, "x.fa") == "\t".join(keys + ["name"]) + "\n3\t3\t2\t1000\t2000\t2000\t3000\t2333\t3000\t6000\tx.fa\n"


def test_record_offsets():
    call = [(b">a\n", [], 3 + 10 + 1), (b">bb 5\n", [], 6 + 0 + 1), (b">c\n", [], 3 + 4 + 1)]
    assert merge.record_offsets(call).tolist() == [0, 3, 13, 20, 20, 24, 28, 29]
    assert merge.record_offsets([]).tolist() == [0, 0]
