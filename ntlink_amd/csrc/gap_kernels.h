/*
 * The cut points of every gap of a grouped result -- what map_long_reads does behind get_accepted_anchor_contigs
 * (bin/ntlink_patch_gaps.py:443-489) as far as it depends on the hits alone: find_orientation and check_position_consistency
 * (:113-127) of the two accepted contigs, the terminal minimizer of each (assess_accepted_anchor_contigs, :492-517) and the cuts
 * assign_read_cut / assign_ctg_cut make of it (:291-308, situations A-D of :276-288).  The fallback and --stringent branches are the
 * host's, over the status word.
 *
 *   gap_cut_kernel   one wavefront per gap, GAP_NT / 64 gaps per workgroup.  Gap g is read g of a grouped result whose group g is
 *                    "contigs 2g and 2g + 1, read g": its mappings are maps[map_off[g] .. map_off[g + 1]) (the scan map_enqueue made
 *                    for its gather), and two mappings are contig 2g (source) and contig 2g + 1 (target) -- a read's accepted
 *                    contigs are distinct -- in the order in which the read meets them: the target first where the read runs against
 *                    the path.
 *
 * The lanes stride over a mapping's hits, in place in the read's region of the hit array; lane j compares hit j with hit j + 1 by
 * loading both, so the loop exchanges nothing between lanes, and four ballots behind it give the four all() of the reference.  Python's
 * all() over an empty zip is True: a mapping of one hit is consistent.  Every loop is bounded by a count read from `maps`, and a record
 * that points outside the arrays (the map kernels make none) is no mapping.
 */
#pragma once
#include "dev_common.h"
#include "map_kernels.h"

#define GAP_NT 256 /* lanes per workgroup: four gaps */

/* bits of GapCut::status (NTL_GAP_* of the ABI) */
#define GAP_NOT_TWO 1u
#define GAP_SRC_MIXED_STRANDS 2u
#define GAP_TGT_MIXED_STRANDS 4u
#define GAP_SRC_POSITIONS 8u
#define GAP_TGT_POSITIONS 16u

struct GapCut { uint32_t status, src_ctg_pos, src_read_cut, src_end_cut, tgt_ctg_pos, tgt_read_cut, tgt_end_cut, ori; }; /* ntl_gap_cut */

struct GapArgs {
    const MapRec *maps; const HitRec *hits; /* the result's dense mappings; the hits in their per-read regions */
    uint64_t maps_cap, hits_cap;            /* records the two arrays hold */
    const uint32_t *map_off;                /* [n_gaps + 1]: first mapping of every read */
    const uint8_t *src_minus, *tgt_minus;   /* [n_gaps]: 1 where the node's sign in the path is '-' */
    uint32_t n_gaps, k;
    GapCut *out;
};

/* The four all() of find_orientation and check_position_consistency over one mapping's hits on one wavefront, the same in every lane
 * (gap_cut_kernel, and gap_select_assess_kernel of gap_select_kernels.h). */
__device__ __forceinline__ void gap_ballots(const HitRec *hits, uint32_t n, uint32_t lane, bool &all_same, bool &all_diff, bool &all_inc, bool &all_dec)
{
    bool same = true, diff = true, inc = true, dec = true;
    for (uint32_t j = lane; j < n; j += 64u) {
        const HitRec h = hits[j];
        same &= h.ctg_strand == h.read_strand;
        diff &= h.ctg_strand != h.read_strand;
        if (j + 1u < n) {
            const uint32_t next = hits[j + 1u].ctg_pos;
            inc &= h.ctg_pos < next;
            dec &= h.ctg_pos > next;
        }
    }
    all_same = __ballot(!same) == 0ull; all_diff = __ballot(!diff) == 0ull;
    all_inc = __ballot(!inc) == 0ull; all_dec = __ballot(!dec) == 0ull;
}

/* One mapping on one wavefront.  Returns the mixed-strands bit (1) and the positions bit (2); plus: the read-based orientation is '+';
 * lane 0 alone holds the terminal hit of a mapping without a flag: `last_if_same` says which end it is when the read-based orientation
 * equals the contig's sign (the source: the last hit, the target: the first). */
__device__ __forceinline__ uint32_t gap_assess(const HitRec *hits, uint32_t n, uint32_t lane, bool ctg_minus, bool last_if_same, bool &plus,
                                               HitRec &terminal)
{
    bool all_same, all_diff, all_inc, all_dec;
    gap_ballots(hits, n, lane, all_same, all_diff, all_inc, all_dec);
    plus = all_same; /* find_orientation asks for '+' first */
    const uint32_t flags = (all_same || all_diff ? 0u : 1u) | (all_inc || all_dec ? 0u : 2u);
    if (lane == 0 && flags == 0) {
        const bool ori_is_sign = plus != ctg_minus;
        terminal = hits[ori_is_sign == last_if_same ? n - 1u : 0u];
    }
    return flags;
}

/* assign_read_cut: the read in '-' on a '+' contig is cut k further on */
__device__ __forceinline__ uint32_t gap_read_cut(uint32_t pos, bool plus, bool ctg_minus, uint32_t k) { return !plus && !ctg_minus ? pos + k : pos; }
/* assign_ctg_cut: a '-' contig with the read-based orientation '-' is cut k further on */
__device__ __forceinline__ uint32_t gap_ctg_cut(uint32_t pos, bool plus, bool ctg_minus, uint32_t k) { return !plus && ctg_minus ? pos + k : pos; }

__global__ __launch_bounds__(GAP_NT) NTL_MAIN_STREAM_SGPRS void gap_cut_kernel(GapArgs A)
{
    NTL_PRIO_LATENCY_BOUND();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = ntl_readfirstlane(blockIdx.x * (GAP_NT / 64u) + (threadIdx.x >> 6)); /* uniform: the loads below are scalar */
    if (g >= A.n_gaps) return;
    const uint32_t m0 = A.map_off[g], nm = A.map_off[g + 1] - m0;
    uint32_t status = GAP_NOT_TWO;
    bool plus[2] = {false, false};
    HitRec term[2] = {};
    const bool minus[2] = {A.src_minus[g] != 0, A.tgt_minus[g] != 0};
    if (nm == 2u && (uint64_t)m0 + 2ull <= A.maps_cap) {
        const MapRec first = A.maps[m0], second = A.maps[m0 + 1u];
        const bool swapped = first.ctg != 2u * g; /* uniform */
        const MapRec S = swapped ? second : first, T = swapped ? first : second;
        const bool inside = S.ctg == 2u * g && T.ctg == 2u * g + 1u && S.n_hits && T.n_hits && S.hit_off + S.n_hits <= A.hits_cap && T.hit_off + T.n_hits <= A.hits_cap;
        if (inside) {
            const uint32_t fs = gap_assess(A.hits + S.hit_off, S.n_hits, lane, minus[0], true, plus[0], term[0]);
            const uint32_t ft = gap_assess(A.hits + T.hit_off, T.n_hits, lane, minus[1], false, plus[1], term[1]);
            status = (fs & 1u ? GAP_SRC_MIXED_STRANDS : 0u) | (fs & 2u ? GAP_SRC_POSITIONS : 0u) |
                     (ft & 1u ? GAP_TGT_MIXED_STRANDS : 0u) | (ft & 2u ? GAP_TGT_POSITIONS : 0u);
        }
    }
    if (lane != 0) return;
    uint4 lo = make_uint4(status, 0u, 0u, 0u), hi = make_uint4(0u, 0u, 0u, 0u);
    if (status == 0u) {
        lo.y = term[0].ctg_pos;
        lo.z = gap_read_cut(term[0].read_pos, plus[0], minus[0], A.k);
        lo.w = gap_ctg_cut(term[0].ctg_pos, plus[0], minus[0], A.k);
        hi.x = term[1].ctg_pos;
        hi.y = gap_read_cut(term[1].read_pos, plus[1], minus[1], A.k);
        hi.z = gap_ctg_cut(term[1].ctg_pos, plus[1], minus[1], A.k);
        hi.w = (plus[0] ? 1u : 0u) | (plus[1] ? 2u : 0u);
    }
    uint4 *o = (uint4 *)&A.out[g];
    o[0] = lo;
    o[1] = hi;
}
