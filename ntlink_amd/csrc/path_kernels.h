/*
 * The graph half of the stitch-paths stage (bin/ntlink_stitch_paths.py:221-365): linearize_graph, is_graph_linear,
 * transitive_filter / has_transitive_support, find_paths / find_paths_process and remove_duplicate_paths on a path graph whose
 * vertices are oriented contigs, v = 2 * contig + (ori == '-'), twin v ^ 1, and that holds every edge with its twin.
 *
 *   path_pass1_kernel      lane per edge: the edge into a table keyed by (src, tgt); per vertex and side (out of src, into tgt)
 *                          the degree, "an edge that is not new is incident", the largest n
 *   path_pass2_kernel      lane per edge: the twin (tgt ^ 1, src ^ 1) is in the table with the same d, n and flags; per vertex
 *                          and side how many edges have the largest n
 *   path_linearize_kernel  lane per edge: the rule of :224-249 at both ends; a kept edge becomes next[src] / prev[tgt]
 *   path_rank_init_kernel, path_rank_round_kernel
 *                          pointer doubling over next[]: (pointer << 32 | distance) in one word per vertex, ping-pong; beside it
 *                          the smallest vertex id met, which names a cycle once the rounds are done
 *   path_support_kernel    lane per scaffold-graph edge (a, b): OR of full / source / target support into the new edges it covers
 *   path_filter_kernel     lane per vertex: a new edge without support goes (:328-352); the graph is ranked again behind it
 *   path_heads_kernel      lane per vertex: cycles counted at their smallest vertex; the head of every chain that is emitted
 *                          gives its length and a one, for the two offset scans
 *   path_scatter_kernel    lane per vertex: (chain, place) -> vertex, the d of the edge behind it, the chain's offset
 *
 * A linear graph is a set of chains and cycles.  After ceil(log2(n_vertices)) rounds the pointer of every chain vertex is its
 * chain's tail (out-degree 0) and the distance its place counted from the tail; a pointer that is no tail belongs to a cycle
 * (find_paths_process finds no source there: the component gives no path).  Of a chain and its twin the one with
 * head <= (tail ^ 1) is emitted; a chain that is its own twin has head == (tail ^ 1).  Plain loads, stores and atomics only.
 */
#pragma once
#include "dev_common.h"

#define PATH_NT 256
#define PATH_NONE 0xFFFFFFFFu
#define PATH_EMPTY 0xFFFFFFFFFFFFFFFFull
#define PATH_EDGE_NEW 1u
#define PATH_MODE_CONSERVATIVE 0u
#define PATH_MODE_STITCH 1u
#define PATH_MODE_TRANSITIVE 2u
#define PATH_ERR_TWIN 1u
#define PATH_ERR_DUP 2u
#define PATH_ERR_NONLINEAR 4u
#define PATH_SUP_FULL 1u
#define PATH_SUP_SOURCE 2u
#define PATH_SUP_TARGET 4u

struct PathEdge { uint32_t src, tgt; int32_t d; uint32_t n, flags; };
struct PathLink { uint32_t a, b; };
/* the first two words are the sums of the two scans (scan_launch's sums_dev), in its order */
struct PathInfo { uint32_t n_chain_vertices, n_chains, removed_linearize, removed_transitive, cycles, err, pad[2]; };

struct PathArgs {
    uint32_t n_vertices, n_edges, n_links, mode;
    const PathEdge *edges;
    const PathLink *links;
    unsigned long long *slots; /* [n_slots] keys (src << 32 | tgt), PATH_EMPTY = free */
    uint32_t *slot_edge;       /* [n_slots] the edge of the key */
    uint32_t slot_bits;
    /* per vertex and side, [2 * v + side]: side 0 = its out-edges, 1 = its in-edges */
    uint32_t *deg, *notnew, *maxn, *cntmax, *kept_deg;
    /* the linear graph, per vertex */
    uint32_t *next, *prev, *vnew, *sup;
    int32_t *vd;               /* d of the edge (v, next[v]) */
    unsigned long long *word[2];
    uint32_t *minv[2];
    uint32_t *head_of;         /* [tail] the head of its chain */
    uint32_t *lens, *cnts;     /* [n_vertices + 1] each, one behind the other: the two scans */
    uint32_t *chain_off, *chain_vertex;
    int32_t *chain_d;
    PathInfo *info;
};

__device__ __forceinline__ uint32_t path_home(unsigned long long key, uint32_t bits)
{
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - bits));
}

__global__ __launch_bounds__(PATH_NT) void path_pass1_kernel(PathArgs A)
{
    const uint32_t i = blockIdx.x * PATH_NT + threadIdx.x;
    if (i >= A.n_edges) return;
    const PathEdge E = A.edges[i];
    const unsigned long long key = (unsigned long long)E.src << 32 | E.tgt;
    const uint32_t mask = (1u << A.slot_bits) - 1u;
    for (uint32_t j = path_home(key, A.slot_bits);; j = (j + 1) & mask) { /* twice as many slots as edges: a free one is met */
        const unsigned long long old = atomicCAS(&A.slots[j], (unsigned long long)PATH_EMPTY, key);
        if (old == PATH_EMPTY) { A.slot_edge[j] = i; break; }
        if (old == key) { atomicOr(&A.info->err, PATH_ERR_DUP); break; }
    }
    const uint32_t so = 2 * E.src, ti = 2 * E.tgt + 1;
    atomicAdd(&A.deg[so], 1u);
    atomicAdd(&A.deg[ti], 1u);
    if (!(E.flags & PATH_EDGE_NEW)) {
        atomicOr(&A.notnew[so], 1u);
        atomicOr(&A.notnew[ti], 1u);
    }
    atomicMax(&A.maxn[so], E.n);
    atomicMax(&A.maxn[ti], E.n);
}

__global__ __launch_bounds__(PATH_NT) void path_pass2_kernel(PathArgs A)
{
    const uint32_t i = blockIdx.x * PATH_NT + threadIdx.x;
    if (i >= A.n_edges) return;
    const PathEdge E = A.edges[i];
    const unsigned long long key = (unsigned long long)(E.tgt ^ 1u) << 32 | (E.src ^ 1u);
    const uint32_t mask = (1u << A.slot_bits) - 1u;
    bool twin = false;
    for (uint32_t j = path_home(key, A.slot_bits);; j = (j + 1) & mask) {
        const unsigned long long k = A.slots[j];
        if (k == PATH_EMPTY) break;
        if (k == key) {
            const PathEdge T = A.edges[A.slot_edge[j]];
            twin = T.d == E.d && T.n == E.n && T.flags == E.flags;
            break;
        }
    }
    if (!twin) atomicOr(&A.info->err, PATH_ERR_TWIN);
    if (E.n == A.maxn[2 * E.src]) atomicAdd(&A.cntmax[2 * E.src], 1u);
    if (E.n == A.maxn[2 * E.tgt + 1]) atomicAdd(&A.cntmax[2 * E.tgt + 1], 1u);
}

/* :224-249 at one end of a new edge: at a branch vertex it stays only if all the edges of that side are new, the largest n is
   unique and it is this edge's */
__device__ __forceinline__ bool path_end_removes(const PathArgs &A, uint32_t side, uint32_t n)
{
    if (A.deg[side] < 2) return false;
    return !(!A.notnew[side] && A.cntmax[side] == 1 && A.maxn[side] == n);
}

__global__ __launch_bounds__(PATH_NT) void path_linearize_kernel(PathArgs A)
{
    const uint32_t i = blockIdx.x * PATH_NT + threadIdx.x;
    if (i >= A.n_edges) return;
    const PathEdge E = A.edges[i];
    const uint32_t so = 2 * E.src, ti = 2 * E.tgt + 1;
    if (A.mode != PATH_MODE_CONSERVATIVE && (E.flags & PATH_EDGE_NEW) && (path_end_removes(A, so, E.n) || path_end_removes(A, ti, E.n))) {
        atomicAdd(&A.info->removed_linearize, 1u);
        return;
    }
    if (atomicAdd(&A.kept_deg[so], 1u) | atomicAdd(&A.kept_deg[ti], 1u)) { /* is_graph_linear, :257-265 */
        atomicOr(&A.info->err, PATH_ERR_NONLINEAR);
        return;
    }
    A.next[E.src] = E.tgt;
    A.prev[E.tgt] = E.src;
    A.vd[E.src] = E.d;
    A.vnew[E.src] = E.flags & PATH_EDGE_NEW;
}

__global__ __launch_bounds__(PATH_NT) void path_rank_init_kernel(PathArgs A)
{
    const uint32_t v = blockIdx.x * PATH_NT + threadIdx.x;
    if (v >= A.n_vertices || A.info->err) return;
    const uint32_t nx = A.next[v];
    A.word[0][v] = nx == PATH_NONE ? (unsigned long long)v << 32 : (unsigned long long)nx << 32 | 1u;
    A.minv[0][v] = v;
}

/* a tail points to itself at distance 0, so a pointer that has arrived stays; on a cycle the distance doubles per round and
   stays below 2^32 for n_vertices < 2^31 */
__global__ __launch_bounds__(PATH_NT) void path_rank_round_kernel(PathArgs A, int from)
{
    const uint32_t v = blockIdx.x * PATH_NT + threadIdx.x;
    if (v >= A.n_vertices || A.info->err) return;
    const unsigned long long w = A.word[from][v];
    const uint32_t p = (uint32_t)(w >> 32);
    const unsigned long long wp = A.word[from][p];
    A.word[from ^ 1][v] = (wp & 0xFFFFFFFF00000000ull) | (uint32_t)((uint32_t)w + (uint32_t)wp);
    const uint32_t a = A.minv[from][v], b = A.minv[from][p];
    A.minv[from ^ 1][v] = a < b ? a : b;
}

__device__ __forceinline__ void path_support_edge(const PathArgs &A, uint32_t a, uint32_t b, uint32_t s)
{
    if (!A.vnew[s]) return;
    const uint32_t t = A.next[s];
    const uint32_t bits = a != s && b != t ? PATH_SUP_FULL : a == s && b == t ? 0u : a == s ? PATH_SUP_SOURCE : PATH_SUP_TARGET;
    if (bits) atomicOr(&A.sup[s], bits);
}

/* `at`: the buffer that holds the finished ranking.  On a chain (a, b) counts when a lies before b, and covers the edges between
   them; on a cycle every vertex is in the in-neighbourhood of every source and the out-neighbourhood of every target (:333-337),
   so it covers the whole cycle */
__global__ __launch_bounds__(PATH_NT) void path_support_kernel(PathArgs A, int at)
{
    const uint32_t i = blockIdx.x * PATH_NT + threadIdx.x;
    if (i >= A.n_links || A.info->err) return;
    const uint32_t a = A.links[i].a, b = A.links[i].b;
    const unsigned long long wa = A.word[at][a], wb = A.word[at][b];
    const uint32_t ta = (uint32_t)(wa >> 32), tb = (uint32_t)(wb >> 32);
    const bool chain_a = A.next[ta] == PATH_NONE, chain_b = A.next[tb] == PATH_NONE;
    if (chain_a && chain_b) {
        if (ta != tb || (uint32_t)wa <= (uint32_t)wb) return;
        uint32_t s = a;
        for (uint32_t left = (uint32_t)wa - (uint32_t)wb; left; left--) {
            path_support_edge(A, a, b, s);
            s = A.next[s];
        }
    } else if (!chain_a && !chain_b && A.minv[at][a] == A.minv[at][b]) {
        uint32_t s = a;
        for (uint32_t left = A.n_vertices; left; left--) { /* a cycle has at most n_vertices edges */
            path_support_edge(A, a, b, s);
            s = A.next[s];
            if (s == a) break;
        }
    }
}

__global__ __launch_bounds__(PATH_NT) void path_filter_kernel(PathArgs A)
{
    const uint32_t s = blockIdx.x * PATH_NT + threadIdx.x;
    if (s >= A.n_vertices || A.info->err) return;
    const uint32_t t = A.next[s];
    if (t == PATH_NONE || !A.vnew[s]) return;
    const uint32_t sup = A.sup[s];
    if ((sup & PATH_SUP_FULL) || (sup & (PATH_SUP_SOURCE | PATH_SUP_TARGET)) == (PATH_SUP_SOURCE | PATH_SUP_TARGET)) return;
    A.next[s] = PATH_NONE; /* only this lane reads next[s] and writes prev[t] here: t has one in-edge */
    A.prev[t] = PATH_NONE;
    atomicAdd(&A.info->removed_transitive, 1u);
}

__global__ __launch_bounds__(PATH_NT) void path_heads_kernel(PathArgs A, int at)
{
    const uint32_t v = blockIdx.x * PATH_NT + threadIdx.x;
    if (v >= A.n_vertices) return;
    uint32_t len = 0;
    if (!A.info->err) {
        const unsigned long long w = A.word[at][v];
        const uint32_t tail = (uint32_t)(w >> 32);
        if (A.next[tail] != PATH_NONE) {
            if (A.minv[at][v] == v) atomicAdd(&A.info->cycles, 1u);
        } else if (A.prev[v] == PATH_NONE && A.next[v] != PATH_NONE) {
            A.head_of[tail] = v;
            if (v <= (tail ^ 1u)) len = (uint32_t)w + 1u;
        }
    }
    A.lens[v] = len;
    A.cnts[v] = len ? 1u : 0u;
}

/* lens and cnts hold their exclusive scans now, the sums at [n_vertices] */
__global__ __launch_bounds__(PATH_NT) void path_scatter_kernel(PathArgs A, int at)
{
    const uint32_t v = blockIdx.x * PATH_NT + threadIdx.x;
    if (v >= A.n_vertices || A.info->err) return;
    if (v == 0) A.chain_off[A.cnts[A.n_vertices]] = A.lens[A.n_vertices];
    const uint32_t nx = A.next[v];
    if (nx == PATH_NONE && A.prev[v] == PATH_NONE) return; /* an isolated vertex is no path (print_paths: fewer than two tokens) */
    const unsigned long long w = A.word[at][v];
    const uint32_t tail = (uint32_t)(w >> 32);
    if (A.next[tail] != PATH_NONE) return;
    const uint32_t h = A.head_of[tail];
    if (h > (tail ^ 1u)) return;
    const uint32_t base = A.lens[h], at_place = base + ((uint32_t)A.word[at][h] - (uint32_t)w);
    A.chain_vertex[at_place] = v;
    A.chain_d[at_place] = nx == PATH_NONE ? 0 : A.vd[v];
    if (v == h) A.chain_off[A.cnts[h]] = base;
}
