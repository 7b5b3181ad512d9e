/*
 * Which read fills which gap -- tally_contig_mapping_info, is_valid_supporting_read with calculate_est_gap_size and
 * find_masking_cut_points of the gap filler (bin/ntlink_patch_gaps.py:149-175, 208-246, 311-342) over one block of
 * <prefix>.verbose_mapping.tsv as the native reader (ntl_vmap_*) delivers it: read r has the mappings maps[map_off[r] ..
 * map_off[r + 1]) in file order, mapping m the hits hits[hit_off .. hit_off + n_hits) and column 3 as anchors[m]; a contig is its
 * number in the caller's name table, GSEL_NO_CTG for a name that is not in it.
 *
 *   gap_select_assess_kernel   per mapping the four all() of find_orientation / check_position_consistency (gap_ballots):
 *                              mstate[m] = 1 (valid) | 2 (orientation '+'); per read `length`, the read_pos of the last hit of the
 *                              last valid mapping (:163).  A read with fewer than two mappings ends before it loads a hit.
 *   gap_select_count_kernel    per read the candidates it gives: every combination i < j of its valid mappings
 *                              (itertools.combinations order) is looked up in the pair table as (i, j) and as
 *                              reverse_complement_pair(i, j), each node carrying the mapping's own orientation.
 *   gap_select_fill_kernel     the same walk behind an exclusive scan of the counts: one 32-byte GapCand per candidate, in the order
 *                              read, combination, direct before reverse complement.  No appending atomic: the place of every record
 *                              is decided by the scan and two ballots.
 *
 * One wavefront per read, GSEL_NT / 64 reads per workgroup, in all three.  The assess kernel strides a mapping's hits over the lanes;
 * the other two take the combinations (i, j0 + lane) of a uniform i in steps of 64.  The pair table is open addressing over 64-bit
 * keys (source node << 32 | target node, node = contig << 1 | minus), empty = all ones, a power of two of slots and at most half
 * full (the host checks both); every probe loop counts its steps and stops at the slot count with GSEL_ERR_PROBE raised, so a wrong
 * table shows as an error, never as a hang.  Two valid mappings of one read on the same contig (a dict overwrite in the reference,
 * never written by `pair`) raise GSEL_ERR_SAME_CTG.  Every loop is bounded by a count read from map_off / maps, and a record that
 * points outside the arrays (the reader makes none) is no mapping, as in gap_cut_kernel.
 */
#pragma once
#include "gap_kernels.h"

#define GSEL_NT 256 /* lanes per workgroup: four reads */

/* bits of GapCand::flags (NTL_GAPSEL_* of the ABI) */
#define GSEL_VALID 1u       /* |gap_est| <= length (is_valid_supporting_read) */
#define GSEL_NEGATIVE 2u    /* a < 0 or b < 0 in calculate_est_gap_size: the reference asserts */
#define GSEL_VIA_REVCOMP 4u /* the pair was found as reverse_complement_pair(i, j) */

#define GSEL_ERR_PROBE 1u    /* bit of *err: a probe sequence did not end within the pair table */
#define GSEL_ERR_SAME_CTG 2u /* bit of *err: two valid mappings of one read name the same contig */

#define GSEL_NO_CTG 0xFFFFFFFFu
#define GSEL_NONE 0xFFFFFFFFu
#define GSEL_EMPTY 0xFFFFFFFFFFFFFFFFull

struct GapCand { uint32_t pair, read, anchors, flags, src_ctg_cut, src_read_cut, tgt_ctg_cut, tgt_read_cut; }; /* ntl_gap_cand */

struct GselArgs {
    const uint32_t *map_off;  /* [n_reads + 1] */
    const MapRec *maps;       /* [n_maps] */
    const uint32_t *anchors;  /* [n_maps] */
    const HitRec *hits;       /* [n_hits] */
    uint64_t n_maps, n_hits;
    uint32_t n_reads, n_ctg, k;
    const uint32_t *ctg_len;  /* [n_ctg] */
    const unsigned long long *pair_keys; /* [n_slots] */
    const uint32_t *pair_vals;           /* [n_slots] */
    uint64_t n_slots;         /* a power of two */
    uint8_t *mstate;          /* [n_maps]: assess -> count, fill */
    uint32_t *length;         /* [n_reads]: assess -> fill */
    uint32_t *cnt;            /* [n_reads + 1]: count writes the candidates of every read, the scan makes offsets of them in place */
    uint32_t *err;
    GapCand *out;
    uint64_t out_cap;         /* records `out` holds (the scan's total) */
};

/* the slot a key's probe sequence starts at; the host builds the table with the same function */
__host__ __device__ inline uint64_t gsel_slot(uint64_t key, uint64_t n_slots) { return ((key * 0x9E3779B97F4A7C15ull) >> 32) & (n_slots - 1ull); }

/* a pair's number, or GSEL_NONE */
__device__ __forceinline__ uint32_t gsel_lookup(const GselArgs &A, uint64_t key, uint32_t &errbits)
{
    uint64_t s = gsel_slot(key, A.n_slots);
    for (uint64_t step = 0; step < A.n_slots; step++) {
        const unsigned long long have = A.pair_keys[s];
        if (have == key) return A.pair_vals[s];
        if (have == GSEL_EMPTY) return GSEL_NONE;
        s = (s + 1ull) & (A.n_slots - 1ull);
    }
    errbits |= GSEL_ERR_PROBE; /* no empty slot: sized wrongly */
    return GSEL_NONE;
}

/* first and end of read r's mappings; false for a read that cannot give a candidate (fewer than two mappings) or whose offsets
 * point outside `maps` */
__device__ __forceinline__ bool gsel_read_maps(const GselArgs &A, uint32_t r, uint32_t &m0, uint32_t &m1)
{
    m0 = A.map_off[r]; m1 = A.map_off[r + 1];
    return m1 > m0 && m1 - m0 >= 2u && (uint64_t)m1 <= A.n_maps;
}

__global__ __launch_bounds__(GSEL_NT) NTL_MAIN_STREAM_SGPRS void gap_select_assess_kernel(GselArgs A)
{
    NTL_PRIO_LATENCY_BOUND();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = ntl_readfirstlane(blockIdx.x * (GSEL_NT / 64u) + (threadIdx.x >> 6)); /* uniform: the loads below are scalar */
    if (r >= A.n_reads) return;
    uint32_t m0, m1, length = 0;
    if (gsel_read_maps(A, r, m0, m1)) {
        for (uint32_t m = m0; m < m1; m++) {
            const MapRec M = A.maps[m];
            uint32_t st = 0;
            const bool inside = M.n_hits && M.hit_off <= A.n_hits && (uint64_t)M.n_hits <= A.n_hits - M.hit_off && (M.ctg == GSEL_NO_CTG || M.ctg < A.n_ctg);
            if (inside) {
                bool all_same, all_diff, all_inc, all_dec;
                gap_ballots(A.hits + M.hit_off, M.n_hits, lane, all_same, all_diff, all_inc, all_dec);
                if ((all_same || all_diff) && (all_inc || all_dec)) {
                    st = 1u | (all_same ? 2u : 0u); /* find_orientation asks for '+' first */
                    length = A.hits[M.hit_off + M.n_hits - 1u].read_pos;
                }
            }
            if (lane == 0) A.mstate[m] = (uint8_t)st;
        }
    }
    if (lane == 0) A.length[r] = length;
}

/* one candidate: the pair as it stands in the path is (S, T) when found directly and (T, S) with both signs flipped when found
 * through its reverse complement; either way the estimate is made from S's last and T's first hit (is_valid_supporting_read swaps
 * back to the read's order), and those two are the terminal hits of find_masking_cut_points as well (:319-329: a source in the read's
 * orientation gives its last hit, a target its first, and the other end each where the orientation differs from the path's sign) */
__device__ __forceinline__ void gsel_emit(const GselArgs &A, uint64_t at, uint32_t pair, uint32_t r, uint32_t length, const MapRec &S, bool s_plus,
                                          uint32_t s_anchors, const MapRec &T, bool t_plus, uint32_t t_anchors, bool via_revcomp)
{
    if (at >= A.out_cap) return;
    const HitRec sl = A.hits[S.hit_off + S.n_hits - 1u], tf = A.hits[T.hit_off];
    const int64_t k = (int64_t)A.k;
    const int64_t a = s_plus ? (int64_t)A.ctg_len[S.ctg] - (int64_t)sl.ctg_pos - k : (int64_t)sl.ctg_pos;
    const int64_t b = t_plus ? (int64_t)tf.ctg_pos : (int64_t)A.ctg_len[T.ctg] - (int64_t)tf.ctg_pos - k;
    const int64_t gap = (int64_t)tf.read_pos - (int64_t)sl.read_pos - a - b;
    const uint32_t flags = ((gap < 0 ? -gap : gap) <= (int64_t)length ? GSEL_VALID : 0u) | (a < 0 || b < 0 ? GSEL_NEGATIVE : 0u) |
                           (via_revcomp ? GSEL_VIA_REVCOMP : 0u);
    const HitRec src = via_revcomp ? tf : sl, tgt = via_revcomp ? sl : tf;
    const bool src_plus = via_revcomp ? t_plus : s_plus, tgt_plus = via_revcomp ? s_plus : t_plus;
    const bool src_minus = via_revcomp ? src_plus : !src_plus, tgt_minus = via_revcomp ? tgt_plus : !tgt_plus; /* the path's signs */
    uint4 *o = (uint4 *)&A.out[at];
    o[0] = make_uint4(pair, r, s_anchors + t_anchors, flags);
    o[1] = make_uint4(gap_ctg_cut(src.ctg_pos, src_plus, src_minus, A.k), gap_read_cut(src.read_pos, src_plus, src_minus, A.k),
                      gap_ctg_cut(tgt.ctg_pos, tgt_plus, tgt_minus, A.k), gap_read_cut(tgt.read_pos, tgt_plus, tgt_minus, A.k));
}

/* the combinations of read r's valid mappings, for counting (FILL false) and for writing the records */
template <bool FILL>
__device__ __forceinline__ void gsel_combinations(const GselArgs &A, uint32_t r, uint32_t lane)
{
    uint32_t m0, m1, total = 0, errbits = 0;
    if (gsel_read_maps(A, r, m0, m1)) {
        const uint64_t base = FILL ? A.cnt[r] : 0u;
        const uint32_t length = FILL ? A.length[r] : 0u;
        for (uint32_t i = m0; i + 1u < m1; i++) { /* uniform */
            const uint32_t si = A.mstate[i];
            if (!(si & 1u)) continue;
            const MapRec S = A.maps[i];
            if (S.ctg == GSEL_NO_CTG) continue; /* a name outside the table matches no pair */
            const uint64_t node_i = ((uint64_t)S.ctg << 1) | (si & 2u ? 0u : 1u);
            for (uint32_t j0 = i + 1u; j0 < m1; j0 += 64u) {
                const uint32_t j = j0 + lane;
                uint32_t direct = GSEL_NONE, revcomp = GSEL_NONE, sj = 0;
                MapRec T = {};
                if (j < m1) {
                    sj = A.mstate[j];
                    T = A.maps[j];
                    if ((sj & 1u) && T.ctg != GSEL_NO_CTG) {
                        if (T.ctg == S.ctg) errbits |= GSEL_ERR_SAME_CTG;
                        else {
                            const uint64_t node_j = ((uint64_t)T.ctg << 1) | (sj & 2u ? 0u : 1u);
                            direct = gsel_lookup(A, (node_i << 32) | node_j, errbits);
                            revcomp = gsel_lookup(A, ((node_j ^ 1ull) << 32) | (node_i ^ 1ull), errbits);
                        }
                    }
                }
                const unsigned long long bd = __ballot(direct != GSEL_NONE), br = __ballot(revcomp != GSEL_NONE);
                if (FILL) {
                    const uint64_t at = base + total + ntl_mbcnt(bd) + ntl_mbcnt(br);
                    if (direct != GSEL_NONE) gsel_emit(A, at, direct, r, length, S, (si & 2u) != 0, A.anchors[i], T, (sj & 2u) != 0, A.anchors[j], false);
                    if (revcomp != GSEL_NONE)
                        gsel_emit(A, at + (direct != GSEL_NONE ? 1u : 0u), revcomp, r, length, S, (si & 2u) != 0, A.anchors[i], T, (sj & 2u) != 0, A.anchors[j], true);
                }
                total += (uint32_t)(__popcll(bd) + __popcll(br));
            }
        }
    }
    if (!FILL && lane == 0) A.cnt[r] = total;
    if (errbits) atomicOr(A.err, errbits);
}

__global__ __launch_bounds__(GSEL_NT) NTL_MAIN_STREAM_SGPRS void gap_select_count_kernel(GselArgs A)
{
    NTL_PRIO_LATENCY_BOUND();
    const uint32_t r = ntl_readfirstlane(blockIdx.x * (GSEL_NT / 64u) + (threadIdx.x >> 6));
    if (r >= A.n_reads) return;
    gsel_combinations<false>(A, r, threadIdx.x & 63u);
}

__global__ __launch_bounds__(GSEL_NT) NTL_MAIN_STREAM_SGPRS void gap_select_fill_kernel(GselArgs A)
{
    NTL_PRIO_LATENCY_BOUND();
    const uint32_t r = ntl_readfirstlane(blockIdx.x * (GSEL_NT / 64u) + (threadIdx.x >> 6));
    if (r >= A.n_reads) return;
    gsel_combinations<true>(A, r, threadIdx.x & 63u);
}
