#!/usr/bin/env python3
"""Golden vectors for the overlap stage behind the filter (ntlink_amd.overlap.merge_overlapping_pathfile and the four writers): the
reference's own ntlink_overlap_sequences and ntlink_utils, imported as the other generators import them, run from
read_fasta_file_trim_prep to print_trimmed_scaffolds on small synthetic assemblies whose contigs really overlap.  Output:
tests/golden/gen/overlapcut_cases.json.gz (data only): per case the inputs (FASTA records, dot file, path file, the k15 w5 minimizer
TSV arranged per path with its LAST marker lines, the arguments) and the end state the reference leaves -- every ScaffoldCut's
orientation, cuts and omit flag, the new paths, the text of the four files.

`igraph` is not installed here; the two modules use a small part of it, which the stand-in below supplies: plain Python written for
this generator (a vertex list, an edge list, a walk for the components, a breadth-first search for the one shortest path).  The
minimizer TSV comes from the oracle's sketch, as in gen_goldens_overlap.py.

main() asserts that the cases reach the branches they were made for.  If a case misses its branch, change the case, not the condition."""
import argparse
import contextlib
import gzip
import io
import json
import os
import sys
import tempfile
import types
from collections import deque

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(REPO, "tests", "golden", "gen", "overlapcut_cases.json.gz")
K, W = 15, 5


# ---------------------------------------------------------------- the igraph stand-in

class InternalError(Exception):
    pass


class _Vertex:
    def __init__(self, graph, index):
        self.graph, self.index = graph, index

    def __getitem__(self, attr):
        return self.graph._vattr[attr][self.index]

    def degree(self):
        return self.graph.degree(self.index)


class _Edge:
    def __init__(self, graph, index):
        self.graph, self.index = graph, index
        self.source, self.target = graph._edges[index]

    def __getitem__(self, attr):
        return self.graph._eattr[attr][self.index]


class _Seq:
    def __init__(self, graph, kind):
        self.graph, self.kind = graph, kind

    def __call__(self):
        return self

    def _attrs(self):
        return self.graph._vattr if self.kind is _Vertex else self.graph._eattr

    def __len__(self):
        return len(self.graph._vattr["name"]) if self.kind is _Vertex else len(self.graph._edges)

    def __iter__(self):
        return (self.kind(self.graph, i) for i in range(len(self)))

    def __getitem__(self, key):
        return self._attrs()[key] if isinstance(key, str) else self.kind(self.graph, key)

    def __setitem__(self, attr, values):
        values = list(values)
        assert len(values) == len(self)
        self._attrs()[attr] = values

    def find(self, name):
        index = self.graph._index.get(name)
        if index is None:
            raise ValueError(f"no such vertex: {name}")
        return _Vertex(self.graph, index)


class Graph:
    def __init__(self, directed=False):
        self.directed = directed
        self._vattr, self._eattr, self._edges, self._index = {"name": []}, {}, [], {}
        self.vs, self.es = _Seq(self, _Vertex), _Seq(self, _Edge)

    def _vid(self, v):
        return v if isinstance(v, int) else self.vs.find(v).index

    def add_vertices(self, names):
        for name in names:
            self._index[name] = len(self._vattr["name"])
            self._vattr["name"].append(name)

    def add_edges(self, pairs):
        for s, t in pairs:
            self._edges.append((self._vid(s), self._vid(t)))
        for values in self._eattr.values():
            values += [None] * (len(self._edges) - len(values))

    def get_eid(self, s, t):
        try:
            s, t = self._vid(s), self._vid(t)
        except ValueError as exc:
            raise InternalError(str(exc))
        for i, (a, b) in enumerate(self._edges):
            if (a, b) == (s, t) or (not self.directed and (b, a) == (s, t)):
                return i
        raise InternalError("no such edge")

    def copy(self):
        g = Graph(self.directed)
        g._vattr = {a: list(v) for a, v in self._vattr.items()}
        g._eattr = {a: list(v) for a, v in self._eattr.items()}
        g._edges, g._index = list(self._edges), dict(self._index)
        return g

    def delete_edges(self, indices):
        gone = set(indices)
        keep = [i for i in range(len(self._edges)) if i not in gone]
        self._edges = [self._edges[i] for i in keep]
        self._eattr = {a: [v[i] for i in keep] for a, v in self._eattr.items()}

    def _neighbours(self):
        out = [[] for _ in self._vattr["name"]]
        for a, b in self._edges:
            out[a].append(b)
            out[b].append(a)
        return out

    def degree(self, v):
        return len(self._neighbours()[v])

    def components(self):
        near, seen, out = self._neighbours(), set(), []
        for v in range(len(near)):
            if v in seen:
                continue
            comp, todo = [], [v]
            seen.add(v)
            while todo:
                u = todo.pop()
                comp.append(u)
                for x in near[u]:
                    if x not in seen:
                        seen.add(x)
                        todo.append(x)
            out.append(sorted(comp))
        return out

    def subgraph(self, vertices):
        vertices = sorted(vertices)
        new = {v: i for i, v in enumerate(vertices)}
        g = Graph(self.directed)
        g._vattr = {a: [vals[v] for v in vertices] for a, vals in self._vattr.items()}
        g._index = {g._vattr["name"][i]: i for i in range(len(vertices))}
        keep = [i for i, (a, b) in enumerate(self._edges) if a in new and b in new]
        g._edges = [(new[self._edges[i][0]], new[self._edges[i][1]]) for i in keep]
        g._eattr = {a: [vals[i] for i in keep] for a, vals in self._eattr.items()}
        return g

    def get_shortest_paths(self, source, target):
        near, before, todo = self._neighbours(), {source: None}, deque([source])
        while todo:
            u = todo.popleft()
            for x in near[u]:
                if x not in before:
                    before[x] = u
                    todo.append(x)
        path = [target]
        while before[path[-1]] is not None:
            path.append(before[path[-1]])
        return [path[::-1]]


igraph = types.ModuleType("igraph")
igraph.Graph, igraph.InternalError = Graph, InternalError
sys.modules["igraph"] = igraph
sys.path.insert(0, os.environ.get("NTLINK_REFERENCE_BIN", "/root/reference/bin"))
sys.path.insert(0, REPO)
import ntlink_overlap_sequences as ref  # noqa: E402  (the reference)
import ntlink_utils  # noqa: E402  (the reference)
import oracle  # noqa: E402


# ---------------------------------------------------------------- the assemblies

REVCOMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(seq):
    return seq.encode().translate(REVCOMP)[::-1].decode()


def assembly(seed):
    """contigs cut from one random genome so that neighbours overlap; -> (records, paths, edges): paths as lists of nodes, edges
    (source node, target node, d)"""
    rng = np.random.default_rng(seed)
    genome = "".join("ACGT"[i] for i in rng.integers(0, 4, 40000))
    other = "".join("ACGT"[i] for i in rng.integers(0, 4, 8000))

    def cut(lo, hi, minus=False):
        return revcomp(genome[lo:hi]) if minus else genome[lo:hi]

    records = [
        # path one, reversed by normalize_path (z... > a...): three contigs in a chain, the middle one '-' and cut at both ends
        ("zeta", cut(0, 2500)), ("mid", cut(2300, 4800, True)), ("alpha", cut(4650, 7000)),
        # path two: a '-' source, an unrelated neighbour (estimated overlap, no shared minimizer), a gap above g + 1, a positive d
        ("b1", cut(8000, 10000, True)), ("b2", cut(9800, 12000)), ("b3", other[:2000]), ("b4", cut(13000, 15000)), ("b5", cut(14900, 17000)),
        ("b6", cut(16950, 19000)),
        # path three: a short contig its predecessor covers whole and its successor shares only the first half of -- the two cuts cross
        # and it is omitted
        ("c1", cut(20000, 22400)), ("c2", cut(22000, 22400)), ("c3", cut(22000, 22200) + other[4500:6800]),
        # path four: two '-' nodes; and a contig no path names
        ("d1", cut(30000, 32000, True)), ("d2", cut(31700, 34000, True)), ("lonely", other[3000:4200]),
    ]
    paths = [["zeta+", "1N", "mid-", "21N", "alpha+"], ["b1-", "21N", "b2+", "5N", "b3+", "300N", "b4+", "21N", "b5+", "21N", "b6+"],
             ["c1+", "21N", "c2+", "21N", "c3+"], ["d1-", "10N", "d2-"]]
    edges = [("zeta+", "mid-", -200), ("mid-", "alpha+", -150), ("alpha-", "mid+", -150), ("mid+", "zeta-", -200),
             ("b1-", "b2+", -200), ("b2+", "b3+", -120), ("b3+", "b4+", -100), ("b4+", "b5+", 40), ("c1+", "c2+", -400), ("c2+", "c3+", -400),
             ("d1-", "d2-", -300)]  # (no edge b5+ -> b6+)
    return records, paths, edges


def sketch_lines(records):
    buf = np.frombuffer("".join(s for _n, s in records).encode(), np.uint8)
    off = np.zeros(len(records) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for _n, s in records])
    mx_off, h, p, _s = oracle.sketch_batch(buf, off, K, W)
    return {name: name + "\t" + " ".join(f"{h[j]}:{p[j]}" for j in range(int(mx_off[i]), int(mx_off[i + 1]))) + "\n"
            for i, (name, _s) in enumerate(records)}


def run_case(name, seed, g, outgap, f):
    records, paths, edges = assembly(seed)
    fasta = "".join(f">{n} some description\n{s}\n" for n, s in records)
    path_text = "".join(f"ntLink_{i}\t{' '.join(p)}\n" for i, p in enumerate(paths))
    nodes = sorted({n for s, t, _d in edges for n in (s, t)} | {n + o for n, _s in records for o in "+-"})
    lengths = dict((n, len(s)) for n, s in records)
    dot = "digraph G {\n" + "graph [scaf_num=7]\n" + "".join(f'"{n}" [l={lengths[n[:-1]]}]\n' for n in nodes) + \
          "".join(f'"{s}" -> "{t}" [d={d} e=100 n=3]\n' for s, t, d in edges) + "}\n"
    lines = sketch_lines(records)
    gap_re = ref.re.compile(r"^(\d+)N$")
    with tempfile.TemporaryDirectory() as tmp:
        files = {"fasta": os.path.join(tmp, "in.fa"), "path": os.path.join(tmp, "in.path"), "d": os.path.join(tmp, "in.dot"), "m": os.path.join(tmp, "in.tsv")}
        for key, text in (("fasta", fasta), ("path", path_text), ("d", dot)):
            with open(files[key], "w") as fh:
                fh.write(text)
        args = argparse.Namespace(m=files["m"], f=f, path=files["path"], fasta=files["fasta"], k=K, d=files["d"], g=g, outgap=outgap + 1,
                                  p=os.path.join(tmp, "out"), v=False, trim_info=True)
        with contextlib.redirect_stdout(io.StringIO()):
            scaffolds = ref.read_fasta_file_trim_prep(args.fasta)
            graph, _ = ntlink_utils.read_scaffold_graph(args.d)
            valid = ntlink_utils.find_valid_mx_regions(args, gap_re, graph, scaffolds)
            # the minimizer stream as ntlink_filter_sequences.py + indexlr make it: per path its contigs with a valid region, then the marker
            tsv = ""
            for i, p in enumerate(paths):
                seen = []
                for node in ntlink_utils.normalize_path(list(p), gap_re):
                    ctg = node.strip("+-")
                    if not ref.re.search(gap_re, node) and ctg in valid and ctg not in seen:
                        seen.append(ctg)
                tsv += "".join(lines[c] for c in seen) + f"LASTntLink_{i}\t\n"
            with open(files["m"], "w") as fh:
                fh.write(tsv)
            new_paths = ref.merge_overlapping_pathfile(args, gap_re, graph, scaffolds, valid)
            ref.print_trim_coordinates(args, scaffolds)
            ref.print_agp_file(new_paths, scaffolds, args)
            ref.print_trimmed_scaffolds(args, scaffolds)
        texts = {suffix: open(f"{args.p}.trimmed_scafs.{suffix}").read() for suffix in ("path", "tsv", "agp", "fa")}
    state = {n: [s.ori, s.source_cut, s.target_cut, s.is_omitted_sequence()] for n, s in scaffolds.items()}
    return {"name": name, "args": {"k": K, "g": g, "outgap": outgap, "f": f}, "fasta": fasta, "path": path_text, "dot": dot, "tsv": tsv,
            "valid": {n: [list(r) for r in regs] for n, regs in valid.items()}, "scaffolds": state, "paths": new_paths, "files": texts}


def main():
    cases = [run_case("g20-outgap0", 11, 20, 0, 0.5), run_case("g20-outgap2", 12, 20, 2, 0.5), run_case("g4-f1", 13, 4, 0, 1.0)]
    first = cases[0]
    st, paths = first["scaffolds"], first["paths"]
    # the branches the cases are there for
    assert st["mid"][0] == "+" and paths["ntLink_0"][0] == "alpha-", "normalize_path reversed the first path"
    assert st["mid"][1] not in (None, 0, 2500) and st["mid"][2] not in (None, 0, 2500), "the middle contig is cut at both ends"
    assert st["b1"][0] == "-" and st["b1"][1] != 0, "a '-' source with a cut (written k further on)"
    assert f"b1\t{st['b1'][1] + K}\t2000\n" in first["files"]["tsv"]
    assert st["b3"][0] is None and "5N b3+" in first["files"]["path"], "an estimated overlap without a shared minimizer: no cut"
    assert "300N" in first["files"]["path"] and st["b4"][0] is None and st["b6"][0] is None, "gap above g + 1, d > 0, no edge"
    assert st["c2"][3] and "c1+ 21N c3+" in first["files"]["path"] and "c2" not in first["files"]["tsv"] and ">c2 " not in first["files"]["fa"]
    assert st["d1"][0] == "-" and st["d2"][0] == "-" and st["d2"][2] != 2300
    assert ">lonely None-None\n" in first["files"]["fa"] and "lonely\t1\t1200\t1\tW\tlonely\t1\t1200\t+\n" in first["files"]["agp"]
    assert " 1N " in first["files"]["path"] and " 3N " in cases[1]["files"]["path"]
    assert "\tN\t2\tscaffold" in cases[1]["files"]["agp"] and "\tN\t" not in first["files"]["agp"].split("ntLink_1")[0]
    assert cases[2]["scaffolds"]["d1"][0] is None, "10N is above g + 1 = 5"
    with gzip.GzipFile(OUT, "wb", mtime=0) as fh:
        fh.write(json.dumps({"cases": cases}).encode())
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
