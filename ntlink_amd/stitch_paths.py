"""The stitch-paths stage: the abyss-scaffold path files of an n sweep to one path file (bin/ntlink_stitch_paths.py, ntLink:233-241).

The host reads the files -- `find_optimal_n`, `read_paths`, `read_alternate_pathfiles` with the four acceptance cases of :140-169,
`add_transitive_support` -- into arrays of oriented contigs, vertex 2 * contig + (ori == '-'), twin v ^ 1; the graph half
(linearize_graph, is_graph_linear, transitive_filter, find_paths, remove_duplicate_paths, :221-365) is one device call,
Device.path_chains (csrc/path_kernels.h); `print_paths` formats its chains.  No igraph, no graph object.

Two differences from the reference.  A best path file in which an oriented contig is a source twice or a target twice is refused:
the reference asserts on the first and, where the assertion does not reach, silently drops such components in find_paths_process.
And with --transitive a contig of a path file that the dot file does not hold is tolerated -- it supports nothing -- where the
reference's scaffold_graph.are_connected raises on the unknown name (it does so in every mode: add_transitive_support runs there
without --transitive too, its result unused)."""
import datetime
import os
import re

import numpy as np

from . import capi
from .overlap import _flip, normalize_path, read_scaffold_graph

NEIGHBOURHOOD = 4  # add_transitive_support's default


def _now():
    return datetime.datetime.today()


def find_optimal_n(path_filenames):
    """The path file whose abyss-scaffold log `<file>.sterr` has the largest N50 (:369-394): files in argument order, 11-column lines
    only, the header line skipped, strictly greater (the first file wins a tie), n from `n=(\\d+)\\s+s=` of the last column."""
    print(_now(), " : Finding optimal n...")
    best_n50, best_n, best_file = 0, 0, None
    n_match = re.compile(r"n=(\d+)\s+s=")
    for path_filename in path_filenames:
        with open(f"{path_filename}.sterr") as path_file:
            for line in path_file:
                line = line.strip().split("\t")
                if len(line) != 11 or line[5] == "N50":
                    continue
                n50 = float(line[5])
                if n50 > best_n50:
                    best_n50, best_n, best_file = n50, int(re.search(n_match, line[10]).group(1)), path_filename
    if best_file is None:
        raise ValueError("no .sterr file reports an N50 above 0: there is no best path file")
    print(_now(), " : Optimal n =", best_n, "at N50 =", best_n50)
    return best_file


class _Names:
    "oriented contig -> vertex, contigs numbered as they are first seen"

    def __init__(self):
        self.number, self.names = {}, []

    def vertex(self, node):
        name = node[:-1]
        c = self.number.get(name)
        if c is None:
            c = self.number[name] = len(self.names)
            self.names.append(name)
        return 2 * c + (node[-1] == "-")

    def node(self, v):
        return self.names[v >> 1] + "+-"[v & 1]


def _path_lines(filename):
    with open(filename) as fh:
        for line in fh:
            path_id, path_sequence = line.strip().split("\t")
            yield path_id, path_sequence.split(" ")


def read_paths(path_filename, names):
    """The best path file as edges (:22-66) -> (src, tgt, d) int arrays holding every edge with its reverse-complement twin: only
    triples whose middle token matches `(\\d+)N` make an edge."""
    print(_now(), ": Building path graph")
    gap_re = re.compile(r"(\d+)N")
    out_of, into = {}, {}
    for _path_id, seq in _path_lines(path_filename):
        for i, j, k in zip(seq, seq[1:], seq[2:]):
            gap_match = re.search(gap_re, j)
            if not gap_match:
                continue
            s, t, d = names.vertex(i), names.vertex(k), int(gap_match.group(1))
            for a, b, what in ((s, t, f"{i} {j} {k}"), (t ^ 1, s ^ 1, f"{i} {j} {k} (reverse complement)")):
                if (a, b) == (s, t) and what.endswith(")"):
                    continue  # X+ gN X-: the edge is its own twin
                if a in out_of or b in into:
                    raise ValueError(f"{path_filename}: {what}: an oriented contig is a source twice or a target twice in the best path file")
                out_of[a], into[b] = (b, d), a
    src = np.fromiter(out_of.keys(), np.int64, len(out_of))
    tgt = np.fromiter((b for b, _d in out_of.values()), np.int64, len(out_of))
    d = np.fromiter((g for _b, g in out_of.values()), np.int64, len(out_of))
    return src, tgt, d


def add_transitive_support(scaffold_edges, path_sequence, connected, neighbourhood=NEIGHBOURHOOD):
    """The extra scaffold-graph edges of one alternate path (:83-118): around every adjacent pair of contigs that the best graph does
    not connect, every (source, target) of the +-4 neighbourhood, both orientations.  A plain loop: the Makefile never passes --transitive."""
    gap_re = re.compile(r"^\d+N$")
    contigs = [node for node in path_sequence if not re.search(gap_re, node)]
    for idx, (s, t) in enumerate(zip(contigs, contigs[1:])):
        if connected(s, t):
            continue
        path = contigs[max(0, idx - neighbourhood):min(len(contigs), idx + neighbourhood + 2)]
        source_idx = path.index(s)
        for source in path[:source_idx + 1]:
            for target in path[source_idx + 1:]:
                if source == s and target == t:
                    continue
                scaffold_edges.add((source, target))
                scaffold_edges.add((_flip(target), _flip(source)))


def read_alternate_pathfiles(path_files, best_filename, names, best, scaffold_edges=None):
    """Every other path file's candidate edges, judged against the BEST file's graph only (:120-219) -> (src, tgt, d, n) of the new
    edges, twins included: d = int(median(gaps)), n = len(gaps) over the accepted candidates of one (source, target).
    best: (src, tgt, d) of read_paths.  scaffold_edges: a set that add_transitive_support fills (--transitive), or None."""
    n_best = len(names.names)
    gap_re = re.compile(r"^(\d+)N$")
    best_edges = set(zip(best[0].tolist(), best[1].tolist()))
    cs, ct, cg = [], [], []

    def connected(s, t):  # a lookup only: a name the best file does not hold is connected to nothing, and gets no number here
        a, b = names.number.get(s[:-1]), names.number.get(t[:-1])
        return a is not None and b is not None and (2 * a + (s[-1] == "-"), 2 * b + (t[-1] == "-")) in best_edges

    for filename in path_files:
        if filename == best_filename:
            continue
        print(f"Reading {filename}")
        if not os.path.exists(filename):
            print(f"{filename} does not exist, skipping.")
            continue
        for _path_id, seq in _path_lines(filename):
            if scaffold_edges is not None:
                add_transitive_support(scaffold_edges, seq, connected)
            for i, j, k in zip(seq, seq[1:], seq[2:]):
                gap_match = re.search(gap_re, j)
                if gap_match:
                    cs.append(names.vertex(i))
                    ct.append(names.vertex(k))
                    cg.append(int(gap_match.group(1)))
    s, t, g = np.array(cs, np.int64), np.array(ct, np.int64), np.array(cg, np.int64)
    # the best graph: which vertices it knows, which have an out-edge / an in-edge
    n_vertices = 2 * len(names.names)
    known = np.zeros(n_vertices, bool)
    known[:2 * n_best] = True  # read_paths adds every vertex with its twin
    has_out, has_in = np.zeros(n_vertices, bool), np.zeros(n_vertices, bool)
    has_out[best[0]], has_in[best[1]] = True, True
    is_connected = np.isin(s * n_vertices + t, best[0] * n_vertices + best[1])
    ks, kt = known[s], known[t]
    accept = (ks & kt & ~is_connected & ~has_out[s] & ~has_in[t]) | (ks & ~kt & ~has_out[s]) | (kt & ~ks & ~has_in[t]) | (~ks & ~kt)
    s, t, g = s[accept], t[accept], g[accept]
    # add_path_edges: both orientations (an edge that is its own twin is appended to twice, as there)
    s, t, g = np.concatenate([s, t ^ 1]), np.concatenate([t, s ^ 1]), np.concatenate([g, g])
    order = np.lexsort((g, t, s))
    s, t, g = s[order], t[order], g[order]
    first = np.flatnonzero(np.r_[True, (s[1:] != s[:-1]) | (t[1:] != t[:-1])]) if len(s) else np.zeros(0, np.int64)
    count = np.diff(np.r_[first, len(s)])
    lo, hi = first + (count - 1) // 2, first + count // 2
    median = (g[lo] + g[hi]) // 2 if len(first) else np.zeros(0, np.int64)  # int(np.median(..)) of gaps that are not negative
    return s[first], t[first], median, count


def format_path_contigs(vertices, gaps, names, max_gap):
    "a chain as path tokens (:267-280): a gap above max_gap + 1 becomes max_gap + 1, -1 for no maximum"
    tokens = []
    for v, gap in zip(vertices[:-1], gaps):
        tokens.append(names.node(v))
        tokens.append(f"{gap if max_gap == -1 or gap <= max_gap + 1 else max_gap + 1}N")
    tokens.append(names.node(vertices[-1]))
    return tokens


def print_paths(paths, out_filename, scaf_num):
    """The path file (:396-420): paths of fewer than two tokens skipped, every path normalised, sorted by (number of tokens, first
    token) descending, ids ntLink_{scaf_num + 1 ..}, from 0 where the dot file says scaf_num=None.  Written beside the output's place
    and renamed when complete."""
    path_id = 0 if scaf_num is None else scaf_num + 1
    gap_re = re.compile(r"\d+N")
    path_lists = [normalize_path(path, gap_re) for path in paths if len(path) >= 2]
    path_lists = sorted(path_lists, key=lambda x: (len(x), x[0]), reverse=True)
    tmp = f"{out_filename}.tmp.{os.getpid()}"
    try:
        with open(tmp, "w") as fout:
            for path_list in path_lists:
                fout.write(f"ntLink_{path_id}\t{' '.join(path_list)}\n")
                path_id += 1
        os.replace(tmp, out_filename)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def stitch_paths(args, dev=None):
    """main() of the reference behind its argument parser (:423-453).  args: the reference's namespace (PATH min_n max_n g a max_gap o p
    transitive conservative).  Writes args.o; after a failure it is not left.  -> the PATH_COUNTS_DT record of the device call."""
    from . import anchor
    dev = dev or anchor._default_device()
    print("Running ntLink stitch paths stage...\n")
    try:
        best_file = find_optimal_n(args.PATH)
        names = _Names()
        best = read_paths(best_file, names)
        scaffold_graph, scaf_num = read_scaffold_graph(args.g)
        if len(best[2]) and int(best[2].max()) >= 1 << 31:
            raise ValueError(f"{best_file}: a gap does not fit 31 bits")
        edges = np.zeros(len(best[0]), capi.PATH_EDGE_DT)
        edges["src"], edges["tgt"], edges["d"] = best
        links, mode = None, capi.NTL_PATH_CONSERVATIVE
        if args.conservative:
            print("Printing paths for optimal N50, no stitching...\n")
        else:
            scaffold_edges = set(scaffold_graph.d) if args.transitive else None
            s, t, d, n = read_alternate_pathfiles(args.PATH, best_file, names, best, scaffold_edges)
            if len(d) and int(d.max()) >= 1 << 31:
                raise ValueError("a gap of an alternate path file does not fit 31 bits")
            new = np.zeros(len(s), capi.PATH_EDGE_DT)
            new["src"], new["tgt"], new["d"], new["n"], new["flags"] = s, t, d, n, capi.NTL_PATH_EDGE_NEW
            edges = np.concatenate([edges, new])
            mode = capi.NTL_PATH_STITCH
            if args.transitive:
                print("Checking for transitive support...\n")
                mode = capi.NTL_PATH_TRANSITIVE
                number = names.number  # an edge with a contig the path graph does not hold supports nothing
                links = np.array([(2 * number[a[:-1]] + (a[-1] == "-"), 2 * number[b[:-1]] + (b[-1] == "-")) for a, b in scaffold_edges
                                  if a[:-1] in number and b[:-1] in number], capi.PATH_LINK_DT).reshape(-1)
        n_vertices = 2 * len(names.names)
        off, vertex, d, counts = dev.path_chains(n_vertices, edges, links, mode)
        print(_now(), ": Finding paths")
        # the weak components of the graph that is left: chains (a lone vertex is one) and cycles; contigs that only a refused
        # candidate named are no vertices of the reference's graph
        used = np.zeros(len(names.names) + 1, bool)
        used[edges["src"] >> 1], used[edges["tgt"] >> 1] = True, True
        left = len(edges) - int(counts["removed_linearize"]) - int(counts["removed_transitive"])
        print("\nTotal number of components in graph:", 2 * int(used.sum()) - left + int(counts["cycles"]), "\n", sep=" ")
        vertex, d, off = vertex.tolist(), d.tolist(), off.tolist()
        paths = [format_path_contigs(vertex[a:b], d[a:b - 1], names, args.max_gap) for a, b in zip(off, off[1:])]
        print_paths(paths, args.o, scaf_num)
    except BaseException:
        if os.path.exists(args.o):
            os.remove(args.o)
        raise
    return counts
