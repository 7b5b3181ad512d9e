"""Crafted path graphs for Device.path_chains and a plain restatement of bin/ntlink_stitch_paths.py:221-365 (linearize_graph,
is_graph_linear, transitive_filter / has_transitive_support, find_paths / find_paths_process, remove_duplicate_paths).

The restatement follows the reference's wording -- a dict of edges with their attributes, incident edges per node, neighbourhoods and
components found by walks, a visited set of contigs -- and knows nothing of ranks, pointers or twins.  What it gives is brought into
the order of the device's contract at the very end: of a path and its reverse complement the one whose head is <= (tail ^ 1), paths
by the number of their head."""
import functools

import numpy as np

from ntlink_amd import capi

CONSERVATIVE, STITCH, TRANSITIVE = capi.NTL_PATH_CONSERVATIVE, capi.NTL_PATH_STITCH, capi.NTL_PATH_TRANSITIVE


class NotLinear(Exception):
    pass


def restated_chains(n_vertices, edges, links, mode):
    """-> (paths [(vertices, gaps)], removed by linearize, removed by the transitive filter, components without a source)"""
    graph = {(s, t): {"d": d, "n": n, "new": bool(flags & 1)} for s, t, d, n, flags in edges}
    scaffold = {(a, b) for a, b in links}

    def incident(g, node, direction):
        return [e for e in g if e[1 if direction == "in" else 0] == node]

    def degrees(g):
        indeg, outdeg = [0] * n_vertices, [0] * n_vertices
        for s, t in g:
            outdeg[s] += 1
            indeg[t] += 1
        return indeg, outdeg

    removed_lin = removed_trans = 0
    if mode != CONSERVATIVE:
        # linearize_graph
        indeg, outdeg = degrees(graph)
        to_remove = set()
        for direction, deg in (("in", indeg), ("out", outdeg)):
            for node in [v for v in range(n_vertices) if deg[v] > 1]:
                max_weight_edge = None
                incident_edges = incident(graph, node, direction)
                if all(graph[e]["new"] for e in incident_edges):
                    max_weight = max(graph[e]["n"] for e in incident_edges)
                    max_weight_edges = [e for e in incident_edges if graph[e]["n"] == max_weight]
                    if len(max_weight_edges) == 1:
                        max_weight_edge = max_weight_edges[0]
                for e in incident_edges:
                    if e != max_weight_edge and graph[e]["new"]:
                        to_remove.add(e)
        graph = {e: a for e, a in graph.items() if e not in to_remove}
        removed_lin = len(to_remove)
    # is_graph_linear (the reference asserts it behind linearize_graph; the best file alone is linear by the stage's own refusal)
    indeg, outdeg = degrees(graph)
    if any(x > 1 for x in indeg) or any(x > 1 for x in outdeg):
        raise NotLinear()
    if mode == TRANSITIVE:
        succ = {s: t for s, t in graph}
        pred = {t: s for s, t in graph}

        def neighbourhood(node, step):
            out, todo = [node], [node]
            while todo:
                v = todo.pop()
                if v in step and step[v] not in out:
                    out.append(step[v])
                    todo.append(step[v])
            return out

        def has_transitive_support(source, target):
            source_pass = target_pass = False
            for test_source in neighbourhood(source, pred):
                for test_target in neighbourhood(target, succ):
                    if test_source == source and test_target == target:
                        continue
                    if (test_source, test_target) in scaffold:
                        if test_source == source or test_target == target:
                            if test_source == source:
                                source_pass = True
                            if test_target == target:
                                target_pass = True
                            if source_pass and target_pass:
                                return True
                        else:
                            return True
            return False

        to_remove = {e for e, a in graph.items() if a["new"] and not has_transitive_support(*e)}
        graph = {e: a for e, a in graph.items() if e not in to_remove}
        removed_trans = len(to_remove)
    # find_paths: the weak components in the order of their lowest vertex, find_paths_process for each
    neighbours = {v: set() for v in range(n_vertices)}
    for s, t in graph:
        neighbours[s].add(t)
        neighbours[t].add(s)
    indeg, outdeg = degrees(graph)
    succ = {s: t for s, t in graph}
    seen, paths, no_source = set(), [], 0
    for v in range(n_vertices):
        if v in seen:
            continue
        component, todo = [], [v]
        seen.add(v)
        while todo:
            u = todo.pop()
            component.append(u)
            for x in neighbours[u] - seen:
                seen.add(x)
                todo.append(x)
        source_nodes = [u for u in component if indeg[u] == 0]
        if len(source_nodes) == 1:
            target_nodes = [u for u in component if outdeg[u] == 0]
            assert len(target_nodes) == 1
            path = [source_nodes[0]]
            while path[-1] != target_nodes[0]:
                path.append(succ[path[-1]])
            if len(path) == len(component) and len(path) == len(set(path)):
                paths.append(path)
        elif not source_nodes:
            no_source += 1
    # remove_duplicate_paths
    visited, kept = set(), []
    for path in paths:
        if not any(u >> 1 in visited for u in path):
            kept.append(path)
        visited.update(u >> 1 for u in path)
    # print_paths skips a path of one contig; then the order of the device's contract
    out = []
    for path in kept:
        if len(path) < 2:
            continue
        gaps = [graph[a, b]["d"] for a, b in zip(path, path[1:])]
        if path[0] > (path[-1] ^ 1):
            path, gaps = [u ^ 1 for u in reversed(path)], gaps[::-1]
        out.append((path, gaps))
    out.sort(key=lambda p: p[0][0])
    return out, removed_lin, removed_trans, no_source


class Graph:
    """edges added with their twins; contigs numbered as they are asked for"""

    def __init__(self):
        self.n_contigs, self.edges, self.links = 0, [], []

    def contigs(self, n):
        first = self.n_contigs
        self.n_contigs += n
        return list(range(first, first + n))

    @property
    def n_vertices(self):
        return 2 * self.n_contigs

    def edge(self, s, t, d=10, n=1, new=False):
        self.edges.append((s, t, d, n, int(new)))
        if (t ^ 1, s ^ 1) != (s, t):
            self.edges.append((t ^ 1, s ^ 1, d, n, int(new)))

    def link(self, a, b):
        self.links.append((a, b))
        if (b ^ 1, a ^ 1) != (a, b):
            self.links.append((b ^ 1, a ^ 1))

    def chain(self, vertices, new=lambda i: False, d=lambda i: 7 + i):
        for i, (s, t) in enumerate(zip(vertices, vertices[1:])):
            self.edge(s, t, d(i), 1, new(i))

    def arrays(self):
        return (np.array(self.edges, capi.PATH_EDGE_DT) if self.edges else np.zeros(0, capi.PATH_EDGE_DT),
                np.array(self.links, capi.PATH_LINK_DT) if self.links else np.zeros(0, capi.PATH_LINK_DT))


def plus(contigs, rng=None):
    "the contigs as vertices, all '+' or with random signs"
    return [2 * c + (int(rng.integers(0, 2)) if rng is not None else 0) for c in contigs]


@functools.lru_cache(maxsize=None)
def crafted():
    """name -> (Graph, mode)"""
    out = {}
    rng = np.random.default_rng(11)
    # chains of every doubling round count up to 11, both sides of a wavefront; the vertices' numbers shuffled along the chain
    for n in (2, 3, 63, 64, 65, 1025):
        g = Graph()
        order = g.contigs(n)
        rng.shuffle(order)
        g.chain(plus(order, rng))
        out[f"chain-{n}"] = (g, STITCH)
    g = Graph()
    for _ in range(300):
        g.chain(plus(g.contigs(2), rng))
    out["chains-300x2"] = (g, STITCH)
    # cycles beside chains
    g = Graph()
    for n in (2, 3, 64):
        ring = plus(g.contigs(n), rng)
        g.chain(ring + ring[:1])
        g.chain(plus(g.contigs(3), rng))
    out["cycles"] = (g, STITCH)
    # a chain that is its own twin: A+ B+ C+ C- B- A- and the odd form A+ B+ B- A- around the edge B+ -> B-
    g = Graph()
    a, b, c = plus(g.contigs(3))
    g.chain([a, b, c, c ^ 1])  # the other half are the twins
    a, b = plus(g.contigs(2))
    g.chain([a ^ 1, b, b ^ 1])
    g.contigs(3)  # isolated vertices
    g.chain(plus(g.contigs(2)))
    out["self-twin"] = (g, STITCH)
    g = Graph()
    g.contigs(5)
    out["isolated-only"] = (g, STITCH)
    # a branch vertex with 2 and with 65 new in-edges: a unique largest n, a tie, and an edge that is not new among them
    for fan in (2, 65):
        for kind in ("unique", "tie", "notnew"):
            g = Graph()
            hub = plus(g.contigs(1))[0]
            g.chain([hub] + plus(g.contigs(2)))
            for i, s in enumerate(plus(g.contigs(fan), rng)):
                n = 3 if i == 0 or (kind == "tie" and i == fan - 1) else 1 + i % 2
                g.edge(s, hub, 5 + i, n, new=not (kind == "notnew" and i == fan - 1))
            out[f"branch-{fan}-{kind}"] = (g, STITCH)
    # --transitive: a chain of 65 whose every second edge is new; scaffold edges spanning 1, 2 and 64 places
    g = Graph()
    v = plus(g.contigs(65), rng)
    g.chain(v, new=lambda i: i % 2 == 1)
    g.link(v[0], v[64])            # full support of every edge but the first and the last
    g.link(v[1], v[3])             # source support of (1, 2)
    g.link(v[0], v[2])             # target support of (1, 2): stays without the long link too
    g.link(v[3], v[4])             # the edge itself: nothing
    g.link(v[63], v[64])
    out["transitive-65"] = (g, TRANSITIVE)
    g = Graph()
    v = plus(g.contigs(12), rng)
    g.chain(v, new=lambda i: i % 2 == 1)
    g.link(v[1], v[3])             # (1, 2): source only -> goes
    g.link(v[2], v[5])             # (3, 4): full
    g.link(v[4], v[6])             # (5, 6): target only -> goes
    g.link(v[7], v[9]); g.link(v[6], v[8])  # (7, 8): source + target
    g.link(v[10], v[9])            # against the chain's direction: nothing; (9, 10) has no support -> goes
    out["transitive-kinds"] = (g, TRANSITIVE)
    # a cycle that the transitive filter opens
    g = Graph()
    ring = plus(g.contigs(5), rng)
    g.chain(ring + ring[:1], new=lambda i: i == 2)
    g.link(ring[2], ring[4])       # a == s alone: source support, the new edge goes and the ring is a chain of 5
    ring = plus(g.contigs(4), rng)
    g.chain(ring + ring[:1], new=lambda i: i == 1)
    g.link(ring[3], ring[0])       # a != s, b != t on a cycle: full support, the cycle stays closed
    out["transitive-cycle"] = (g, TRANSITIVE)
    g = Graph()
    g.chain(plus(g.contigs(4)), new=lambda i: True)
    out["conservative"] = (g, CONSERVATIVE)
    return out


def random_graph(g, rng, n_contigs):
    """a symmetric graph on new contigs: chains and rings of not-new edges, then new edges between random ends and a few into the
    middle of a chain (branches that linearize removes), with scaffold edges along and across"""
    contigs = g.contigs(n_contigs)
    rng.shuffle(contigs)
    v = plus(contigs, rng)
    pieces, at = [], 0
    while at < len(v):
        n = int(rng.integers(1, 9))
        pieces.append(v[at:at + n])
        at += n
    have = set()

    def edge(s, t, n, new):
        if s >> 1 == t >> 1 or (s, t) in have or (t ^ 1, s ^ 1) in have:
            return
        have.update({(s, t), (t ^ 1, s ^ 1)})
        g.edge(s, t, int(rng.integers(0, 500)), n, new)

    for p in pieces:
        for s, t in zip(p, p[1:]):
            edge(s, t, 1, rng.random() < 0.3)
        if len(p) > 2 and rng.random() < 0.15:
            edge(p[-1], p[0], 1, rng.random() < 0.5)  # a ring
    for _ in range(len(pieces)):
        a, b = pieces[int(rng.integers(len(pieces)))], pieces[int(rng.integers(len(pieces)))]
        s = a[-1] if rng.random() < 0.8 else a[int(rng.integers(len(a)))]
        t = b[0] if rng.random() < 0.8 else b[int(rng.integers(len(b)))]
        if rng.random() < 0.3:
            s, t = t ^ 1, s ^ 1
        edge(s, t, int(rng.integers(1, 4)), True)
    for _ in range(2 * len(pieces)):
        p = pieces[int(rng.integers(len(pieces)))]
        q = p if rng.random() < 0.7 else pieces[int(rng.integers(len(pieces)))]
        g.link(p[int(rng.integers(len(p)))], q[int(rng.integers(len(q)))])
        if rng.random() < 0.5:
            g.link(p[-1], pieces[int(rng.integers(len(pieces)))][0])


@functools.lru_cache(maxsize=None)
def random_batches():
    """200 random graphs of at most 200 vertices, 25 to a call as one disjoint union (a launch under the SIMT mock costs a thread per
    lane whatever the graph's size): [(Graph, mode)]"""
    rng = np.random.default_rng(2027)
    out = []
    for batch in range(8):
        g = Graph()
        for _ in range(25):
            random_graph(g, rng, int(rng.integers(1, 101)))
        g.links = sorted(set(g.links))
        out.append((g, (STITCH, TRANSITIVE)[batch % 2]))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    g, mode = crafted()[name] if isinstance(name, str) else random_batches()[name]
    return restated_chains(g.n_vertices, g.edges, g.links, mode)


def run(dev, g, mode):
    edges, links = g.arrays()
    return dev.path_chains(g.n_vertices, edges, links, mode)


def compare(dev, name):
    g, mode = crafted()[name] if isinstance(name, str) else random_batches()[name]
    paths, removed_lin, removed_trans, no_source = expected(name)
    off, vertex, d, counts = run(dev, g, mode)
    got = [(vertex[a:b].tolist(), d[a:b - 1].tolist()) for a, b in zip(off[:-1].tolist(), off[1:].tolist())]
    assert len(off) == int(counts["n_chains"]) + 1 and int(off[-1]) == len(vertex) == int(counts["n_chain_vertices"]), name
    assert all(int(d[b - 1]) == 0 for b in off[1:].tolist()), name
    assert len(got) == len(paths), f"{name}: {len(got)} chains, the restated reference gives {len(paths)}"
    for i, (a, b) in enumerate(zip(got, paths)):
        assert a == b, f"{name}: chain {i} is {a}, the restated reference gives {b}"
    assert (int(counts["removed_linearize"]), int(counts["removed_transitive"]), int(counts["cycles"])) == (removed_lin, removed_trans, no_source), name
    return paths, removed_lin, removed_trans, no_source
