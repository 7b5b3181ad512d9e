/*
 * Liftover of a resident map result through an AGP (ntl_mapres_liftover): liftover_ctg_mappings and print_adjusted_mappings of
 * bin/ntlink_liftover_mappings.py:61-121 over the records of a result instead of the lines of <prefix>.verbose_mapping.tsv.  The host
 * form of the same work is ntl_liftover.cpp; DESIGN 4.11 has the semantics and the argument for the regions.
 *
 *   lift_line_kernel      one wavefront per mapping (one input line), LIFT_NT / 64 mappings per workgroup, in rounds of 64 hits: the
 *                         range filter, the shift or the mirror, and the kept hits compacted in order (ballot + ntl_mbcnt ranks) into a
 *                         second hit array at the line's own hit_off.  Per line: the output name, the kept count, the first and the last
 *                         kept position, and whether the kept positions strictly increase / strictly decrease.  A kept hit meets its
 *                         predecessor through 64 words of LDS per wavefront (the rank before it; the last of the round before).
 *   lift_read_kernel      one lane per LINE; the lane of a read's first line (the line before it names another read, or there is
 *                         none) does that read: runs by name, subsumption by name, groups, monotonicity across the joins
 *                         (lift_read_body).  A read of more than LIFT_LANE_LINES lines goes on a list instead.
 *   lift_read_overflow_kernel   one wavefront per listed read, the same body: the two quadratic steps are spread over the lanes,
 *                         the walk along the groups stays with lane 0.
 *   (scan_launch over the per-line `emit` words: the output number of every group)
 *   lift_gather_kernel    one wavefront per line: the hits of a line of an emitted group move to `region start of the group's first
 *                         line + the line's offset in the group`; the group's first line writes the mapping.
 *
 * Every loop is bounded by a count the kernel was given (n_maps, a mapping's n_hits, a read's number of lines, the list's length);
 * a mapping whose hit region leaves the hit array is no mapping (flag LIFT_ERR_REGION: the makers of a result produce none).
 */
#pragma once
#include "dev_common.h"
#include "map_kernels.h"

#define LIFT_NT 256          /* lanes per workgroup of the per-line kernels: four mappings */
#define LIFT_LANE_LINES 16u  /* lines of one read a single lane walks (NTL_LIFT_LANE_LINES of the ABI); more: the overflow kernel */
#define LIFT_OVER_BLOCKS 1024u /* wavefronts of the overflow kernel; each takes every LIFT_OVER_BLOCKS-th listed read */

#define LIFT_ERR_CTG 1u     /* a mapping's ctg is not below n_ctg */
#define LIFT_ERR_RANGE 2u   /* a lifted position does not fit 32 bits */
#define LIFT_ERR_REGION 4u  /* a mapping's hit region leaves the hit array */

struct LiftEntry { uint32_t new_ctg, mode, scaf_start, ctg_start, ctg_end; }; /* ntl_lift_entry */
struct LiftLine { uint32_t name, kept, first, last; }; /* per input line: output name, kept hits, first / last kept (lifted) position */
struct LiftInfo { uint32_t err, n_over; unsigned long long n_hits; }; /* error bits, listed reads, hits of the emitted groups */

struct LiftArgs {
    const MapRec *maps; const HitRec *hits; /* the input result: dense mappings, hits in their regions */
    uint64_t hits_cap;                      /* slots of `hits`, of `kept_hits` and of `out_hits` */
    uint32_t n_maps, n_ctg;
    int32_t k;
    const LiftEntry *table;                 /* [n_ctg] */
    HitRec *kept_hits;                      /* the kept, lifted hits of line m from maps[m].hit_off on */
    LiftLine *line;                         /* [n_maps] */
    uint8_t *mono;                          /* [n_maps] bit 0: the kept positions strictly increase, bit 1: strictly decrease */
    uint8_t *cov, *drop;                    /* [n_maps] the line lies strictly between the first and a later run of some name; its name is subsumed */
    uint32_t *gfirst, *goff, *gcnt;         /* [n_maps] first line of the line's group (NTL_NONE: dropped), hits of the group in front of
                                               the line; of a group's first line: the group's hits when it is emitted, else 0 */
    uint32_t *emit;                         /* [n_maps + 1] 1 for the first line of an emitted group; scanned: the output number */
    uint32_t *over_list;                    /* [n_maps] first lines of the reads of more than LIFT_LANE_LINES lines */
    LiftInfo *info;
    MapRec *out_maps; HitRec *out_hits;
};

__global__ __launch_bounds__(LIFT_NT) NTL_MAIN_STREAM_SGPRS void lift_line_kernel(LiftArgs A)
{
    NTL_PRIO_LATENCY_BOUND();
    __shared__ uint32_t s_pos[LIFT_NT / 64][64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t m = ntl_readfirstlane(blockIdx.x * (LIFT_NT / 64u) + w); /* uniform */
    if (m >= A.n_maps) return;
    const MapRec M = A.maps[m];
    uint32_t err = 0u, n = M.n_hits;
    LiftEntry E = {NTL_NONE, 0u, 1u, 1u, 1u};
    if (M.ctg < A.n_ctg) E = A.table[M.ctg]; else err |= LIFT_ERR_CTG;
    if (M.hit_off > A.hits_cap || (uint64_t)n > A.hits_cap - M.hit_off) { err |= LIFT_ERR_REGION; n = 0u; }
    if (E.mode == 0u || err) n = 0u; /* not in the AGP: the line stays for the grouping, its hits go */
    const int64_t k = A.k, lo = (int64_t)E.ctg_start - 1, hi = (int64_t)E.ctg_end - k;
    const int64_t len = (int64_t)E.ctg_end - (int64_t)E.ctg_start + 1, offset = (int64_t)E.scaf_start - 1;
    const HitRec *src = A.hits + M.hit_off;
    HitRec *dst = A.kept_hits + M.hit_off;
    uint32_t kept = 0u, first = 0u, last = 0u;
    bool inc = true, dec = true, wide = false;
    for (uint32_t base = 0u; base < n; base += 64u) { /* uniform */
        const uint32_t j = base + lane;
        HitRec h = {};
        if (j < n) h = src[j];
        const int64_t p = h.ctg_pos;
        const bool keep = j < n && p >= lo && p <= hi;
        int64_t q = p;
        if (E.mode == 2u) q = offset + (p - lo);
        else if (E.mode == 3u) { q = offset + (len - (p - lo)) - k; h.ctg_strand ^= 1u; }
        if (keep && q > 0xFFFFFFFFll) wide = true;
        const uint32_t q32 = (uint32_t)q;
        const unsigned long long mask = __ballot(keep);
        const uint32_t rank = ntl_mbcnt(mask), cnt = (uint32_t)__popcll(mask);
        if (keep) {
            h.ctg_pos = q32;
            dst[kept + rank] = h;
            s_pos[w][rank] = q32;
        }
        ntl_wave_sync();
        if (keep && (rank || kept)) {
            const uint32_t prev = rank ? s_pos[w][rank - 1u] : last;
            inc &= prev < q32;
            dec &= prev > q32;
        }
        if (cnt) {
            if (!kept) first = s_pos[w][0];
            last = s_pos[w][cnt - 1u];
        }
        ntl_wave_sync(); /* the next round writes s_pos again */
        kept += cnt;
    }
    const bool all_inc = __ballot(!inc) == 0ull, all_dec = __ballot(!dec) == 0ull, any_wide = __ballot(wide) != 0ull;
    if (lane != 0u) return;
    if (any_wide) err |= LIFT_ERR_RANGE;
    if (err) atomicOr(&A.info->err, err);
    *(uint4 *)&A.line[m] = make_uint4(E.new_ctg, kept, first, last);
    A.mono[m] = (uint8_t)((all_inc ? 1u : 0u) | (all_dec ? 2u : 0u));
}

/* One read = the L lines from line m0 on.  WAVE: the 64 lanes of a workgroup of one wavefront share the read (lines lane, lane + 64,
 * ...), with a workgroup barrier between the steps, which pass their results through cov[] and drop[]; otherwise one lane does it all.
 *
 * print_adjusted_mappings (:89-121) groups the lines into runs of one name, keeps the index of every name's FIRST run, and lets a later
 * run of a known name mark the name of every run strictly between the two as subsumed.  The runs between a name's first run and ANY
 * later run of it lie between its first and its LAST run, so per name p one interval of lines does it: behind the end of p's first run,
 * in front of the start of p's last run.
 *   1. per name (the lane of its first line): that interval into cov[]
 *   2. per line: drop[] = some line of the same name is covered -- subsumption goes by name, so p may subsume itself (A B A C A) and
 *      two names each other (A B A B)
 *   3. along the lines that stay: groups of consecutive lines of one name; a group's positions are strictly monotonic iff every line's
 *      are (mono[]) and every join -- last kept position of one line, first kept position of the next line that kept any -- steps the
 *      same way.  The first line of a group that holds a hit and is monotonic is marked in emit[]. */
template <bool WAVE>
__device__ __forceinline__ void lift_read_body(const LiftArgs &A, uint32_t m0, uint32_t L, uint32_t lane)
{
    const uint32_t step = WAVE ? 64u : 1u;
    const LiftLine *ln = A.line + m0;
    uint8_t *cov = A.cov + m0, *drop = A.drop + m0;
    for (uint32_t i = lane; i < L; i += step) cov[i] = 0u;
    if (WAVE) __syncthreads();
    for (uint32_t i = lane; i < L; i += step) {
        const uint32_t p = ln[i].name;
        bool seen = false;
        for (uint32_t a = 0u; a < i && !seen; a++) seen = ln[a].name == p;
        if (seen) continue; /* not the first line of p's first run */
        uint32_t e = i;
        while (e + 1u < L && ln[e + 1u].name == p) e++; /* the last line of the first run */
        uint32_t t = L - 1u;
        while (t > e && ln[t].name != p) t--; /* the last line of p */
        if (t == e) continue; /* no later run */
        uint32_t s = t;
        while (ln[s - 1u].name == p) s--; /* the first line of the last run: line e + 1 is not p's, so s >= e + 2 */
        for (uint32_t l = e + 1u; l < s; l++) cov[l] = 1u; /* (several names may cover a line: every one stores 1) */
    }
    if (WAVE) __syncthreads();
    for (uint32_t i = lane; i < L; i += step) {
        const uint32_t p = ln[i].name;
        bool sub = false;
        for (uint32_t a = 0u; a < L && !sub; a++) sub = cov[a] != 0u && ln[a].name == p;
        drop[i] = sub ? 1u : 0u;
    }
    if (WAVE) __syncthreads();
    if (lane != 0u) return;
    unsigned long long hits = 0ull;
    uint32_t i = 0u;
    while (i < L) {
        A.emit[m0 + i] = 0u; A.gcnt[m0 + i] = 0u;
        if (drop[i]) { A.gfirst[m0 + i] = NTL_NONE; i++; continue; }
        const uint32_t p = ln[i].name, f = i;
        uint32_t total = 0u, prev = 0u, j = i;
        bool inc = true, dec = true, have = false;
        while (j < L) {
            if (j != f) { A.emit[m0 + j] = 0u; A.gcnt[m0 + j] = 0u; }
            if (drop[j]) { A.gfirst[m0 + j] = NTL_NONE; j++; continue; }
            const LiftLine X = ln[j];
            if (X.name != p) break;
            A.gfirst[m0 + j] = m0 + f; A.goff[m0 + j] = total;
            if (X.kept) {
                const uint32_t mono = A.mono[m0 + j];
                inc = inc && (mono & 1u) != 0u && (!have || prev < X.first);
                dec = dec && (mono & 2u) != 0u && (!have || prev > X.first);
                prev = X.last; have = true;
                total += X.kept;
            }
            j++;
        }
        if (total && (inc || dec)) { A.emit[m0 + f] = 1u; A.gcnt[m0 + f] = total; hits += total; }
        i = j;
    }
    if (hits) atomicAdd(&A.info->n_hits, hits);
}

/* A read = a run of consecutive mappings with equal .read.  The lines of the read from line m on, counted no further than limit + 1
 * (limit + 1: "more than limit"). */
__device__ __forceinline__ uint32_t read_lines_from(const MapRec *maps, uint32_t n_maps, uint32_t m, uint32_t limit)
{
    const uint32_t read = maps[m].read;
    uint32_t L = 1u;
    while (L <= limit && m + L < n_maps && maps[m + L].read == read) L++;
    return L;
}

/* ... and 0 where line m is not a read's first line (the line before it names the same read) */
__device__ __forceinline__ uint32_t read_lines_at_first(const MapRec *maps, uint32_t n_maps, uint32_t m, uint32_t limit)
{
    if (m && maps[m - 1u].read == maps[m].read) return 0u;
    return read_lines_from(maps, n_maps, m, limit);
}

__global__ __launch_bounds__(LIFT_NT) void lift_read_kernel(LiftArgs A)
{
    const uint32_t m = blockIdx.x * LIFT_NT + threadIdx.x;
    if (m >= A.n_maps) return;
    const uint32_t L = read_lines_at_first(A.maps, A.n_maps, m, LIFT_LANE_LINES);
    if (!L) return; /* not a read's first line */
    if (L > LIFT_LANE_LINES) { A.over_list[atomicAdd(&A.info->n_over, 1u)] = m; return; }
    lift_read_body<false>(A, m, L, 0u);
}

__global__ __launch_bounds__(64) void lift_read_overflow_kernel(LiftArgs A)
{
    const uint32_t n_over = A.info->n_over; /* at most n_maps / (LIFT_LANE_LINES + 1) */
    for (uint32_t o = blockIdx.x; o < n_over && o < A.n_maps; o += gridDim.x) { /* uniform */
        const uint32_t m = A.over_list[o];
        const uint32_t L = read_lines_from(A.maps, A.n_maps, m, NTL_NONE); /* uniform */
        lift_read_body<true>(A, m, L, threadIdx.x);
        __syncthreads();
    }
}

/* Regions cannot overlap.  A group's lines l1 < l2 < ... have only dropped lines between them (a line of another name that stays
 * would have ended the group), and dropped lines belong to no group; the next group's first line lies behind this group's last one.
 * The group writes at most as many hits as its lines kept, and a line keeps at most the hits it had, so the group stays inside
 * [hit_off of l1, end of the region of its last line), and the input's regions ascend with the line number without overlapping
 * (ntl_mapres_from_host, map_gather_kernel): the spans of two groups are disjoint, and the output's regions ascend with the output
 * number.  The source is the second hit array, not the destination: no line reads what another wrote. */
__global__ __launch_bounds__(LIFT_NT) NTL_MAIN_STREAM_SGPRS void lift_gather_kernel(LiftArgs A)
{
    NTL_PRIO_LATENCY_BOUND();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t m = ntl_readfirstlane(blockIdx.x * (LIFT_NT / 64u) + (threadIdx.x >> 6)); /* uniform */
    if (m >= A.n_maps) return;
    const uint32_t f = A.gfirst[m];
    if (f == NTL_NONE || f > m) return;
    const uint32_t total = A.gcnt[f];
    if (!total) return; /* the group is empty or not monotonic */
    const MapRec F = A.maps[f];
    const uint32_t kept = A.line[m].kept, off = A.goff[m];
    if (off > total || kept > total - off || F.hit_off + total > A.hits_cap) return; /* (what lift_read_body wrote never does) */
    const HitRec *src = A.kept_hits + A.maps[m].hit_off;
    HitRec *dst = A.out_hits + F.hit_off + off;
    for (uint32_t j = lane; j < kept; j += 64u) dst[j] = src[j];
    if (m == f && lane == 0u) {
        MapRec O = F;
        O.ctg = A.line[f].name; O.n_hits = total; O.pad = 0u;
        A.out_maps[A.emit[f]] = O;
    }
}
