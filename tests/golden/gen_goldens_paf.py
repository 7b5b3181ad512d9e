#!/usr/bin/env python3
"""Golden vectors for the PAF block path: the reference's own print_paf (bin/ntlink_paf_output.py:103-135), imported in the build
container, over the crafted runs of tests/paf_cases.py (the small stencil cases, the thresholds and votes, the seam runs) and the first
50 runs of its random sweep -- one accepted contig per call, its hits in read order.
Output: tests/golden/gen/paf_blocks.json.gz (data only: the hits that went in, the fields of the lines that came out).
Same import recipe as tests/golden/gen_goldens.py."""
import gzip
import io
import json
import os
import sys
import types

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.modules["igraph"] = types.ModuleType("igraph")
sys.path.insert(0, "/root/reference/bin")
import ntlink_paf_output  # noqa: E402  (the reference)
import ntlink_utils  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tests"))
import paf_cases  # noqa: E402

GEN = os.path.join(REPO, "tests", "golden", "gen")
CTG_LEN = 100000


def main():
    cases, n_lines = [], 0
    for name, hits in paf_cases.fixture_cases():
        run = types.SimpleNamespace(contig="ctg", hits=[ntlink_utils.MinimizerPositions(mx=str(i), ctg_pos=cp, ctg_strand="+-"[cs], read_pos=rp,
                                                                                         read_strand="+-"[rs])
                                                        for i, (cp, rp, cs, rs) in enumerate(hits)])
        read_len = hits[-1][1] + 1000
        out = io.StringIO()
        ntlink_paf_output.print_paf(out, {"ctg": run}, read_len, "read", {"ctg": ntlink_utils.Scaffold(id="ctg", length=CTG_LEN)}, paf_cases.K)
        paf = []
        for line in out.getvalue().splitlines():
            f = line.split("\t")
            assert f[0] == "read" and int(f[1]) == read_len and f[5] == "ctg" and int(f[6]) == CTG_LEN and f[11] == "255"
            assert int(f[10]) == int(f[8]) - int(f[7])
            paf.append([int(f[2]), int(f[3]), int(f[7]), int(f[8]), int(f[9]), f[4]])
        assert [h[1] for h in hits] == [paf_cases.RSTEP * i for i in range(len(hits))]
        cases.append({"name": name, "ctg_pos": [h[0] for h in hits], "ctg_strand": "".join(str(h[2]) for h in hits),
                      "read_strand": "".join(str(h[3]) for h in hits), "paf": paf})
        n_lines += len(paf)
    doc = {"k": paf_cases.K, "read_step": paf_cases.RSTEP, "fields": ["q_start", "q_end", "t_start", "t_end", "n_hits", "strand"], "cases": cases}
    with open(os.path.join(GEN, "paf_blocks.json.gz"), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as fh:
        fh.write(json.dumps(doc, separators=(",", ":")).encode())
    print(len(cases), "cases,", n_lines, "lines")


if __name__ == "__main__":
    main()
