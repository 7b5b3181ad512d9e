/*
 * The pair records of a resident map result (ntl_mapres_pairs): the per-read part of tally_add<false> of ntl_pairs.cpp -- which pairs of
 * a read's mappings are evaluated, in which order, with which orientation, gap and anchor flag, and which are dropped
 * (tally_pairs_from_mappings, calculate_pair_info, calculate_gap_size, normalize_pair of bin/ntlink_pair.py) -- over the records where
 * they lie.  The dictionary keyed by pair, which depends on the order across reads, stays on the host (ntl_tally_add_pairs).  DESIGN 4.13
 * has the semantics and the order argument.
 *
 *   pair_line_kernel            one lane per mapping: its first and last hit from its region, the contig's rank and length, the two
 *                               overhangs (a: behind the last hit, as a pair's source; b: in front of the first, as its target), the two
 *                               orientations, "more than one hit".  A mapping the table or the hit array does not hold raises a flag.
 *   pair_read_kernel<EMIT>      one lane per LINE; the lane of a read's first line does that read (pair_read_body) when it has at most
 *                               PAIR_LANE_MAPS lines, and puts it on a list otherwise.  EMIT = false counts the read's records into
 *                               cnt[first line], EMIT = true writes them from the scanned cnt[first line] on: one body, so that the two
 *                               passes cannot disagree.
 *   pair_read_overflow_kernel<EMIT>   one wavefront per listed read, the same body: the lanes share every list of pairs in rounds of 64,
 *                               a kept pair's place among its round's is its rank in the ballot.
 *   (scan_launch over cnt[] between the two passes)
 *
 * Every loop is bounded by a count the kernel was given (n_maps, a read's number of lines, the list's length); a record is written
 * below out_cap only.
 */
#pragma once
#include "dev_common.h"
#include "map_kernels.h"
#include "liftover_kernels.h" /* read_lines_from, read_lines_at_first: the reads are found the way the liftover finds them */

#define PAIR_NT 256           /* lanes per workgroup of the per-line kernels */
#define PAIR_LANE_MAPS 16u    /* mappings of one read a single lane walks (NTL_PAIR_LANE_MAPS of the ABI); more: the overflow kernel */
#define PAIR_OVER_BLOCKS 1024u /* wavefronts of the overflow kernel; each takes every PAIR_OVER_BLOCKS-th listed read */
#define PAIR_MAX_RECS 0xFFFFFF00ull /* 2^32 - 256: a result of so many records or more is refused */

#define PAIR_ERR_CTG 1u       /* a mapping's ctg is not below n_ctg */
#define PAIR_ERR_READ 2u      /* a mapping's read is not below n_reads (only with a read_len array) */
#define PAIR_ERR_REGION 4u    /* a mapping has no hit, or its hit region leaves the hit array */
#define PAIR_ERR_NEGATIVE 8u  /* an overhang of an evaluated pair is negative: "Gap distance estimation less than 0" */

#define PAIR_F_SRC_PLUS 1u    /* PairLine.flags: orientation as a source (from the last hit), as a target (from the first), n_hits > 1 */
#define PAIR_F_TGT_PLUS 2u
#define PAIR_F_STRONG 4u

struct PairRec { uint32_t src, tgt; int64_t gap; uint32_t read; uint8_t src_ori, tgt_ori, anchor, pad; }; /* ntl_pair_rec */
struct PairCtg { uint32_t rank, len; }; /* per contig: dense rank of its name (ntl_tally_create), its length */
struct PairLine { int64_t a, b; uint32_t first_rp, last_rp, rank, flags; };
struct PairInfo { uint32_t err, n_over; unsigned long long total; }; /* error bits, listed reads, records of the whole result */

struct PairArgs {
    const MapRec *maps; const HitRec *hits; /* the result: dense mappings, hits in their regions */
    uint64_t hits_cap;                      /* slots of `hits` */
    uint32_t n_maps, n_ctg;
    int32_t k, f;
    const PairCtg *table;                   /* [n_ctg] */
    const uint32_t *read_len;               /* [n_reads], or null: the largest read_pos among the first and last hits of the read's mappings */
    uint64_t n_reads;
    PairLine *line;                         /* [n_maps] */
    uint64_t *key1;                         /* [n_maps] of line i of a chain read: the key of the neighbour pair (i, i + 1) if it was recorded, else 0 */
    uint32_t *cnt;                          /* [n_maps + 1] records of the read whose first line this is (0 for every other line); scanned: where they start */
    uint32_t *over_list;                    /* [n_maps] first lines of the reads of more than PAIR_LANE_MAPS lines */
    PairInfo *info;
    PairRec *out; uint64_t out_cap;
};

__global__ __launch_bounds__(PAIR_NT) void pair_line_kernel(PairArgs A)
{
    const uint32_t m = blockIdx.x * PAIR_NT + threadIdx.x;
    if (m >= A.n_maps) return;
    const MapRec M = A.maps[m];
    uint32_t err = 0u;
    if (M.ctg >= A.n_ctg) err |= PAIR_ERR_CTG;
    if (A.read_len && M.read >= A.n_reads) err |= PAIR_ERR_READ;
    if (!M.n_hits || M.hit_off > A.hits_cap || (uint64_t)M.n_hits > A.hits_cap - M.hit_off) err |= PAIR_ERR_REGION;
    PairLine P = {};
    if (!err) {
        const HitRec hf = A.hits[M.hit_off], hl = A.hits[M.hit_off + M.n_hits - 1u];
        const PairCtg T = A.table[M.ctg];
        const int64_t clen = T.len, k = A.k;
        const bool sp = hl.read_strand == hl.ctg_strand, tp = hf.read_strand == hf.ctg_strand;
        P.a = sp ? clen - (int64_t)hl.ctg_pos - k : (int64_t)hl.ctg_pos;
        P.b = tp ? (int64_t)hf.ctg_pos : clen - (int64_t)hf.ctg_pos - k;
        P.first_rp = hf.read_pos; P.last_rp = hl.read_pos; P.rank = T.rank;
        P.flags = (sp ? PAIR_F_SRC_PLUS : 0u) | (tp ? PAIR_F_TGT_PLUS : 0u) | (M.n_hits > 1u ? PAIR_F_STRONG : 0u);
    } else atomicOr(&A.info->err, err);
    A.line[m] = P;
}

struct PairEval { uint64_t key; PairRec rec; bool keep; }; /* keep: the pair is recorded unless the key check of the second list says otherwise */

/* add_pair of mappings mi (source) and mj (target) of one read, up to the dictionary: calculate_gap_size with its assertion,
 * normalize_pair by the rank of the names (equal ranks swap), the key of ntl_pairs.cpp, and the |gap| > read length rule. */
__device__ __forceinline__ PairEval pair_eval(const PairArgs &A, uint32_t mi, uint32_t mj, uint32_t read, int64_t rl, uint32_t &err)
{
    const PairLine X = A.line[mi], Y = A.line[mj];
    PairEval O = {};
    if (X.a < 0 || Y.b < 0) { err |= PAIR_ERR_NEGATIVE; return O; } /* before either drop rule, as in the reference */
    const int64_t gap = (int64_t)Y.first_rp - (int64_t)X.last_rp - X.a - Y.b;
    uint32_t ci = A.maps[mi].ctg, cj = A.maps[mj].ctg, ri = X.rank, rj = Y.rank;
    uint32_t so = X.flags & PAIR_F_SRC_PLUS ? 1u : 0u, to = Y.flags & PAIR_F_TGT_PLUS ? 1u : 0u;
    if (!(ri < rj)) { /* smaller name first, both orientations flipped */
        uint32_t x = ci; ci = cj; cj = x;
        x = ri; ri = rj; rj = x;
        x = so; so = to ^ 1u; to = x ^ 1u;
    }
    O.key = ((uint64_t)ri << 33) | ((uint64_t)so << 32) | ((uint64_t)rj << 1) | to | (1ull << 63);
    O.keep = (gap < 0 ? -gap : gap) <= rl;
    O.rec.src = ci; O.rec.tgt = cj; O.rec.gap = gap; O.rec.read = read;
    O.rec.src_ori = (uint8_t)so; O.rec.tgt_ori = (uint8_t)to;
    O.rec.anchor = (X.flags & Y.flags & PAIR_F_STRONG) ? 1u : 0u;
    return O;
}

/* One read = the L >= 1 lines from line m0 on.  WAVE: the 64 lanes of a workgroup of one wavefront share every list of pairs in rounds
 * of 64 (every lane takes part in every ballot: the loops are uniform); otherwise one lane does it all, in the order of the host's loop.
 *
 *   L <= f     every (i, j), i < j, in itertools.combinations order
 *   otherwise  the neighbours (i, i + 1); then, per line i of more than one hit, (i, t) with t the next such line -- the neighbours among
 *              the strong lines, in the order of i -- unless a neighbour pair of this read was recorded under the same key (key1[]).
 *              Where t == i + 1 the pair IS the neighbour pair: recorded, its key is in the list; dropped or refused, it would be
 *              dropped or refused again; so it is not evaluated a second time.
 * (f is compared as the host compares it, converted to 64 bits unsigned: a negative f sends every read down the first branch.) */
template <bool WAVE, bool EMIT>
__device__ __forceinline__ void pair_read_body(const PairArgs &A, uint32_t m0, uint32_t L, uint32_t lane)
{
    const uint32_t step = WAVE ? 64u : 1u;
    const PairLine *ln = A.line + m0;
    const uint32_t read = A.maps[m0].read;
    int64_t rl = 0;
    if (A.read_len) { if (read < A.n_reads) rl = A.read_len[read]; }
    else { /* the checkpoint rule */
        uint32_t mx = 0u;
        for (uint32_t i = lane; i < L; i += step) {
            const uint32_t p = ln[i].first_rp > ln[i].last_rp ? ln[i].first_rp : ln[i].last_rp;
            mx = p > mx ? p : mx;
        }
        if (WAVE) mx = ~ntl_wave_min(~mx);
        rl = mx;
    }
    const uint64_t base = EMIT ? A.cnt[m0] : 0ull;
    uint64_t n = 0ull; /* records of this read so far (the same in every lane) */
    uint32_t err = 0u;
    auto put = [&](bool ok, const PairEval &O) {
        uint32_t rank = 0u, c = ok ? 1u : 0u;
        if (WAVE) {
            const unsigned long long mask = __ballot(ok);
            rank = ntl_mbcnt(mask); c = (uint32_t)__popcll(mask);
        }
        if (EMIT && ok) {
            const uint64_t at = base + n + rank;
            if (at < A.out_cap) A.out[at] = O.rec;
        }
        n += c;
    };
    if ((uint64_t)L <= (uint64_t)(int64_t)A.f) {
        for (uint32_t i = 0u; i + 1u < L; i++)
            for (uint32_t jb = i + 1u; jb < L; jb += step) { /* uniform */
                const uint32_t j = jb + lane;
                PairEval O = {};
                if (j < L) O = pair_eval(A, m0 + i, m0 + j, read, rl, err);
                put(O.keep, O);
            }
    } else {
        for (uint32_t ib = 0u; ib + 1u < L; ib += step) { /* uniform */
            const uint32_t i = ib + lane;
            PairEval O = {};
            if (i + 1u < L) {
                O = pair_eval(A, m0 + i, m0 + i + 1u, read, rl, err);
                A.key1[m0 + i] = O.keep ? O.key : 0ull;
            }
            put(O.keep, O);
        }
        if (WAVE) __syncthreads(); /* key1[] of this read is complete */
        for (uint32_t ib = 0u; ib + 1u < L; ib += step) { /* uniform */
            const uint32_t i = ib + lane;
            PairEval O = {};
            if (i + 1u < L && (ln[i].flags & PAIR_F_STRONG)) {
                uint32_t t = i + 1u;
                while (t < L && !(ln[t].flags & PAIR_F_STRONG)) t++;
                if (t < L && t != i + 1u) {
                    O = pair_eval(A, m0 + i, m0 + t, read, rl, err);
                    for (uint32_t q = 0u; q + 1u < L && O.keep; q++) O.keep = A.key1[m0 + q] != O.key;
                }
            }
            put(O.keep, O);
        }
    }
    if (err) atomicOr(&A.info->err, err);
    if (!EMIT && lane == 0u) {
        A.cnt[m0] = n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n; /* (the total refuses the result then) */
        if (n) atomicAdd(&A.info->total, (unsigned long long)n);
    }
}

/* the emit pass of a result that is refused writes nothing */
__device__ __forceinline__ bool pair_refused(const PairArgs &A) { return A.info->err != 0u || A.info->total >= PAIR_MAX_RECS; }

template <bool EMIT>
__global__ __launch_bounds__(PAIR_NT) void pair_read_kernel(PairArgs A)
{
    const uint32_t m = blockIdx.x * PAIR_NT + threadIdx.x;
    if (m >= A.n_maps) return;
    if (EMIT && pair_refused(A)) return;
    const uint32_t L = read_lines_at_first(A.maps, A.n_maps, m, PAIR_LANE_MAPS);
    if (!EMIT && (!L || L > PAIR_LANE_MAPS)) A.cnt[m] = 0u; /* (the overflow kernel, which runs behind this one, counts a listed read) */
    if (!L) return; /* not a read's first line */
    if (L > PAIR_LANE_MAPS) {
        if (!EMIT) A.over_list[atomicAdd(&A.info->n_over, 1u)] = m;
        return;
    }
    pair_read_body<false, EMIT>(A, m, L, 0u);
}

template <bool EMIT>
__global__ __launch_bounds__(64) void pair_read_overflow_kernel(PairArgs A)
{
    if (EMIT && pair_refused(A)) return; /* uniform */
    const uint32_t n_over = A.info->n_over; /* at most n_maps / (PAIR_LANE_MAPS + 1) */
    for (uint32_t o = blockIdx.x; o < n_over && o < A.n_maps; o += gridDim.x) { /* uniform */
        const uint32_t m = A.over_list[o];
        const uint32_t L = read_lines_from(A.maps, A.n_maps, m, NTL_NONE); /* uniform */
        pair_read_body<true, EMIT>(A, m, L, threadIdx.x);
    }
}
