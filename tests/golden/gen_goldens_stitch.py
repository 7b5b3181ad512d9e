#!/usr/bin/env python3
"""Golden vectors for the stitch-paths stage (ntlink_amd.stitch_paths): the reference's own ntlink_stitch_paths and ntlink_utils,
imported as the other generators import them, run from find_optimal_n to print_paths on small crafted path files.  Output:
tests/golden/gen/stitch_cases.json.gz (data only): per case the path files, their .sterr files, the dot file, the arguments and the
text of the output file.

`igraph` is not installed here; the two modules use a small part of it, which the stand-in below supplies: plain Python written for
this generator (a vertex list, an edge list, walks for components, neighbourhoods and the one shortest path).  Scaffold graphs hold
every edge with its twin, as the pair stage writes them.

main() asserts that the cases reach the branches they were made for.  If a case misses its branch, change the case, not the condition.
One branch cannot be reached from files: a branch vertex with an edge that is not new on the branching side.  A candidate is accepted
only at an out-end (in-end) of the best graph, so a vertex that gets new out-edges (in-edges) has no old one; tests/path_cases.py has
that case on the edge list itself."""
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

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(REPO, "tests", "golden", "gen", "stitch_cases.json.gz")


# ---------------------------------------------------------------- the igraph stand-in (directed)

class InternalError(Exception):
    pass


class _Vertex:
    def __init__(self, graph, index):
        self.graph, self.index = graph, index

    def __getitem__(self, attr):
        return self.graph._vattr[attr][self.index]

    def indegree(self):
        return sum(1 for _s, t in self.graph._edges if t == self.index)

    def outdegree(self):
        return sum(1 for s, _t in self.graph._edges if s == self.index)


class _Edge:
    def __init__(self, graph, index):
        self.graph, self.index = graph, index
        self.source, self.target = graph._edges[index]

    def __getitem__(self, attr):
        return self.graph._eattr[attr][self.index]

    def __setitem__(self, attr, value):
        self.graph._eattr.setdefault(attr, [None] * len(self.graph._edges))[self.index] = value


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


IN, OUT_MODE = 2, 1


class Graph:
    def __init__(self, directed=False):
        assert directed
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

    def ecount(self):
        return len(self._edges)

    def get_eid(self, s, t):
        s, t = self._vid(s), self._vid(t)
        for i, edge in enumerate(self._edges):
            if edge == (s, t):
                return i
        raise InternalError("no such edge")

    def are_connected(self, s, t):
        return (self._vid(s), self._vid(t)) in set(self._edges)  # an unknown name raises ValueError, as igraph does

    def incident(self, node, mode=OUT_MODE):
        return [i for i, (s, t) in enumerate(self._edges) if (t if mode == IN else s) == node]

    def copy(self):
        g = Graph(True)
        g._vattr = {a: list(v) for a, v in self._vattr.items()}
        g._eattr = {a: list(v) for a, v in self._eattr.items()}
        g._edges, g._index = list(self._edges), dict(self._index)
        return g

    def delete_edges(self, indices):
        gone = set(indices)
        keep = [i for i in range(len(self._edges)) if i not in gone]
        self._edges = [self._edges[i] for i in keep]
        self._eattr = {a: [v[i] for i in keep] for a, v in self._eattr.items()}

    def _step(self, mode):
        out = [[] for _ in self._vattr["name"]]
        for a, b in self._edges:
            if mode in ("out", "all"):
                out[a].append(b)
            if mode in ("in", "all"):
                out[b].append(a)
        return out

    def components(self, mode="weak"):
        assert mode == "weak"
        near, seen, out = self._step("all"), set(), []
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
        g = Graph(True)
        g._vattr = {a: [vals[v] for v in vertices] for a, vals in self._vattr.items()}
        g._index = {g._vattr["name"][i]: i for i in range(len(vertices))}
        keep = [i for i, (a, b) in enumerate(self._edges) if a in new and b in new]
        g._edges = [(new[self._edges[i][0]], new[self._edges[i][1]]) for i in keep]
        g._eattr = {a: [vals[i] for i in keep] for a, vals in self._eattr.items()}
        return g

    def _walk(self, source, mode, order=None):
        near, depth, todo = self._step(mode), {source: 0}, deque([source])
        before = {source: None}
        while todo:
            u = todo.popleft()
            if order is not None and depth[u] >= order:
                continue
            for x in near[u]:
                if x not in depth:
                    depth[x], before[x] = depth[u] + 1, u
                    todo.append(x)
        return depth, before

    def get_shortest_paths(self, source, target):
        _depth, before = self._walk(source, "out")
        if target not in before:
            return [[]]
        path = [target]
        while before[path[-1]] is not None:
            path.append(before[path[-1]])
        return [path[::-1]]

    def neighborhood(self, vertex, order=1, mode="all"):
        depth, _before = self._walk(self._vid(vertex), mode, order)
        return list(depth)


igraph = types.ModuleType("igraph")
igraph.Graph, igraph.InternalError, igraph.IN, igraph.OUT = Graph, InternalError, IN, OUT_MODE
sys.modules["igraph"] = igraph
sys.path.insert(0, os.environ.get("NTLINK_REFERENCE_BIN", "/root/reference/bin"))
import ntlink_stitch_paths as ref  # noqa: E402  (the reference)


# ---------------------------------------------------------------- the cases

def sterr(n, n50, junk=True):
    text = "Reading something\n" if junk else ""
    text += "n\tn:500\tL50\tmin\tN75\tN50\tN25\tE-size\tmax\tsum\tname\n"
    text += f"30\t25\t5\t1000\t2000\t{n50}\t4000\t3500\t9000\t90000\tn={n} s=1000\n"
    return text


def dot(contigs, edges, scaf_num):
    lines = ["digraph G {"] + [f'"{c}{o}" [l=1000]' for c in contigs for o in "+-"]
    flip = lambda v: v[:-1] + ("-" if v[-1] == "+" else "+")
    for s, t in edges:
        lines.append(f'"{s}" -> "{t}" [d=10 e=0 n=3]')
        if (flip(t), flip(s)) != (s, t):
            lines.append(f'"{flip(t)}" -> "{flip(s)}" [d=10 e=0 n=3]')
    return "\n".join(lines + [f"graph [scaf_num={scaf_num}]", "}"]) + "\n"


def paths_text(lines):
    return "".join(f"{i}\t{line}\n" for i, line in enumerate(lines))


def contigs_of(*texts):
    out = []
    for text in texts:
        for line in text.splitlines():
            for tok in line.split("\t")[1].split(" "):
                if tok[-1] in "+-" and tok[:-1] not in out:
                    out.append(tok[:-1])
    return out


BEST = ["a+ 10N b+ 20N c+", "d+ 5N e-", "f+ g+ h+", "x+ 7N y+", "lone+"]
ALT1 = ["c+ 30N d+",                 # both known, out-end and in-end: accepted
        "a+ 9N b+",                  # connected already
        "b+ 9N d+",                  # both known, b+ is no out-end
        "e- 15N k+",                 # the source known and an out-end, the target new
        "a+ 15N m+",                 # the source known, no out-end
        "n+ 12N a+",                 # the target known and an in-end, the source new
        "q+ 12N b+",                 # the target known, no in-end
        "r+ 8N s+ 3N t+",            # neither known
        "z+ 5N d+",                  # a second edge into d+: an in-branch with a unique largest n (c+ -> d+ is seen three times)
        "u+ 4N v+", "r+ 50N o+"]     # r+ -> s+ twice, r+ -> o+ once: an out-branch with a unique largest n
ALT3 = ["c+ 33N d+ 2N e-", "r+ 9N s+", "u+ 6N w+"]   # u+ -> v+ and u+ -> w+ once each: a tie, both go
ALT4 = ["c+ 40N d+"]

ACCEPTED = {("c+", "d+"): [30, 33, 40], ("e-", "k+"): [15], ("n+", "a+"): [12], ("r+", "s+"): [8, 9], ("s+", "t+"): [3], ("z+", "d+"): [5],
            ("u+", "v+"): [4], ("r+", "o+"): [50], ("u+", "w+"): [6]}


def stitch_files(scaf_num, links=()):
    files = {"s.n1.path": paths_text(ALT1), "s.n2.path": paths_text(BEST), "s.n3.path": paths_text(ALT3), "s.n4.path": paths_text(ALT4),
             "s.n1.path.sterr": sterr(1, 2500), "s.n2.path.sterr": sterr(2, 3000), "s.n3.path.sterr": sterr(3, 3000, junk=False),  # a tie: n2 is first
             "s.n4.path.sterr": sterr(4, 100), "s.n5.path.sterr": sterr(5, 2999)}                                                 # s.n5.path is missing
    files["g.dot"] = dot(contigs_of(*(files[f] for f in files if f.endswith(".path"))), links, scaf_num)
    return files, ["s.n1.path", "s.n2.path", "s.n3.path", "s.n4.path", "s.n5.path"]


T_BEST = ["a+ 10N b+", "c+ 10N d+", "e+ 10N f+", "g+ 10N h+", "i+ 10N j+"]
T_ALT = ["b+ 5N c+", "d+ 5N e+", "f+ 5N g+", "h+ 5N i+"]
T_LINKS = [("a+", "d+"),                 # b+ -> c+: full support
           ("d+", "f+"), ("c+", "e+"),   # d+ -> e+: source and target
           ("f+", "h+")]                 # f+ -> g+: source only; h+ -> i+: nothing
T2_BEST = ["a+ 10N b+", "c+ 10N d+"]
T2_ALT = ["a+ 10N b+ 5N c+ 10N d+"]      # add_transitive_support gives (a+, d+): b+ -> c+ stays without any scaffold edge


def cases():
    out = {}

    def case(name, files, paths, g="g.dot", max_gap=-1, transitive=False, conservative=False):
        out[name] = {"files": files, "args": {"PATH": paths, "min_n": 1, "max_n": 5, "g": g, "a": 0.3, "max_gap": max_gap, "transitive": transitive,
                                              "conservative": conservative}}

    files, paths = stitch_files(17)
    case("stitch", files, paths)
    case("conservative", files, paths, conservative=True)
    for max_gap in (4, 9, 1000):  # below every gap but the smallest; 10 == max_gap + 1 stays; above all
        case(f"stitch-max_gap-{max_gap}", files, paths, max_gap=max_gap)
    files, paths = stitch_files("None")
    case("stitch-scaf_num-none", files, paths)
    files = {"t.n1.path": paths_text(T_BEST), "t.n2.path": paths_text(T_ALT), "t.n1.path.sterr": sterr(1, 5000), "t.n2.path.sterr": sterr(2, 4000)}
    files["g.dot"] = dot(contigs_of(files["t.n1.path"], files["t.n2.path"]), T_LINKS, 3)
    case("transitive", files, ["t.n1.path", "t.n2.path"], transitive=True)
    case("transitive-off", files, ["t.n1.path", "t.n2.path"])
    files = {"t.n1.path": paths_text(T2_BEST), "t.n2.path": paths_text(T2_ALT), "t.n1.path.sterr": sterr(1, 5000), "t.n2.path.sterr": sterr(2, 4000)}
    files["g.dot"] = dot(contigs_of(files["t.n1.path"]), [], 0)
    case("transitive-added", files, ["t.n1.path", "t.n2.path"], transitive=True)
    files = dict(files)
    files["t.n2.path"] = paths_text(["b+ 5N c+"])
    case("transitive-none", files, ["t.n1.path", "t.n2.path"], transitive=True)
    return out


def run_reference(case, accepted):
    with tempfile.TemporaryDirectory() as tmp:
        for name, text in case["files"].items():
            with open(os.path.join(tmp, name), "w") as fh:
                fh.write(text)
        a = case["args"]
        argv = [os.path.join(tmp, p) for p in a["PATH"]] + ["--min_n", str(a["min_n"]), "--max_n", str(a["max_n"]), "-g", os.path.join(tmp, a["g"]),
                                                            "-a", str(a["a"]), "--max_gap", str(a["max_gap"]), "-o", os.path.join(tmp, "out.path")]
        argv += ["--transitive"] * a["transitive"] + ["--conservative"] * a["conservative"]
        original = ref.NtLinkPath.add_path_edges

        def logged(gap_dist, source, target, new_edges):
            accepted.setdefault((source, target), []).append(gap_dist)
            return original(gap_dist, source, target, new_edges)

        ref.NtLinkPath.add_path_edges, old_argv, stdout = staticmethod(logged), sys.argv, io.StringIO()
        sys.argv = ["ntlink_stitch_paths.py"] + argv
        try:
            with contextlib.redirect_stdout(stdout):
                try:
                    ref.main()
                except SystemExit as exc:
                    assert exc.code == 0
        finally:
            sys.argv, ref.NtLinkPath.add_path_edges = old_argv, staticmethod(original)
        with open(os.path.join(tmp, "out.path")) as fh:
            return fh.read(), stdout.getvalue().replace(tmp + os.sep, "")


def main():
    argparse.ArgumentParser(description=__doc__).parse_args()
    all_cases = cases()
    for name, case in all_cases.items():
        accepted = {}
        case["output"], stdout = run_reference(case, accepted)
        lines = [line.split("\t")[1] for line in case["output"].splitlines()]
        if name.startswith("stitch"):
            assert accepted == ACCEPTED, (name, accepted)  # the four acceptance cases, every refusal, edges seen in 1, 2 and 3 files
            assert "Optimal n = 2 at N50 = 3000.0" in stdout and "s.n5.path does not exist, skipping." in stdout, stdout
            assert case["output"].startswith("ntLink_0\t" if "none" in name else "ntLink_18\t"), case["output"]
            mg = case["args"]["max_gap"]
            gap = lambda g: f"{g if mg == -1 or g <= mg + 1 else mg + 1}N"  # 10 == 9 + 1 stays at max_gap 9
            flip = lambda path: " ".join(t if t.endswith("N") else t[:-1] + ("-" if t[-1] == "+" else "+") for t in reversed(path.split(" ")))
            has = lambda path: path in lines or flip(path) in lines
            assert has(f"n+ {gap(12)} a+ {gap(10)} b+ {gap(20)} c+ {gap(33)} d+ {gap(5)} e- {gap(15)} k+"), lines  # median 33 of three; z+ -> d+ lost
            assert has(f"r+ {gap(8)} s+ {gap(3)} t+"), lines                                                     # median 8.5 -> 8; r+ -> o+ lost
            assert not any("u+" in line or "u-" in line or "z+" in line or "z-" in line or "o+" in line or "o-" in line for line in lines), lines  # the tie; the in-branch's loser
            assert has(f"x+ {gap(7)} y+") and not any("f+" in line or "lone" in line for line in lines), lines
            assert (gap(20), gap(10)) == {-1: ("20N", "10N"), 4: ("5N", "5N"), 9: ("10N", "10N"), 1000: ("20N", "10N")}[mg]
        if name == "conservative":
            assert not accepted and lines == ["a+ 10N b+ 20N c+", "x+ 7N y+", "d+ 5N e-"], lines
        if name == "transitive":
            assert lines == ["a+ 10N b+ 5N c+ 10N d+ 5N e+ 10N f+", "i+ 10N j+", "g+ 10N h+"], lines
        if name == "transitive-off":
            assert lines == ["a+ 10N b+ 5N c+ 10N d+ 5N e+ 10N f+ 5N g+ 10N h+ 5N i+ 10N j+"], lines
        if name == "transitive-added":
            assert lines == ["a+ 10N b+ 5N c+ 10N d+"], lines
        if name == "transitive-none":
            assert lines == ["c+ 10N d+", "a+ 10N b+"], lines
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with gzip.GzipFile(OUT, "wb", mtime=0) as fh:
        fh.write(json.dumps(all_cases, indent=0, sort_keys=True).encode())
    print(f"wrote {OUT}: {len(all_cases)} cases")


if __name__ == "__main__":
    main()
