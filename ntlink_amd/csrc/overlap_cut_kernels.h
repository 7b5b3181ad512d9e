/*
 * The cut points of adjacent, overlapping contigs: merge_overlapping of bin/ntlink_overlap_sequences.py:341-417 with
 * filter_minimizers_position (:304-322), is_valid_pos (:297-301) and get_dist_from_end (:335-339), on the kept minimizers
 * ntl_overlap_filter leaves (per sequence: unique hashes, position order).
 *
 * The reference builds a graph per pair: a vertex per minimizer the two slices share, an edge between neighbours of either list, and
 * keeps the edges both lists have (weight 2, filter_graph_global).  Both lists hold the same unique keys, so a kept edge joins two
 * keys that are neighbours in the SOURCE list and neighbours in the target list: the kept edges are a subset of the source list's
 * own path edges, and a component is a run of consecutive shared minimizers in source order whose target ranks step by +1 or -1
 * (one sign per run: the ranks are distinct).  No graph is needed:
 *
 *   slices     each side's part of its sequence's kept list with start <= pos <= end: two binary searches on the position
 *   shared     a source minimizer whose hash is in the target slice (an open-addressing table of the target slice, keyed by the hash;
 *              an empty slot is marked by its INDEX word, the all-ones hash is a key like any other)
 *   ranks      source rank r: exclusive scan of the shared flags in source order; target rank: the same scan in target order
 *   runs       rank r heads a run iff r == 0 or |trank[r] - trank[r - 1]| != 1; the run number is the scan of the heads
 *   score      the lane at a run's tail scores it.  One minimizer: mapped_region_length 1, mid_mx itself.  Two or more: the path
 *              is walked from the end whose hash is the smaller DECIMAL STRING (the reference compares vertex names, :367-369),
 *              mid_mx = path[len // 2] in that direction, mapped_region_length = median of the two spans; in both cases
 *              median_length_from_end = median of the two get_dist_from_end values.  A median of two integers is half their sum:
 *              the sums are compared, in integers.
 *   best       maximum of (mapped_region_length, median_length_from_end, mid_mx as a string) (:407-408): a tree over the workgroup.
 *              The cuts are mid_mx's two positions.
 *
 *   overlap_cut_kernel           one workgroup of OVC_NT lanes per pair; every per-pair array in LDS.  A pair whose target slice
 *                                holds more than OVC_LDS_SLICE minimizers is put on the overflow list and left alone.
 *   overlap_cut_overflow_kernel  the same body (ovc_pair) for the pairs of that list, a workgroup's arrays in its slab of a global
 *                                scratch buffer sized for the longest listed slice.
 *
 * OVC_LDS_SLICE = 1024: 2048 table slots of 12 bytes and three rank arrays of 1024 words, 36 KB of the CU's 160 KB, so four
 * workgroups (16 wavefronts) stay resident per CU.  At k15 w5 a contig end gives about one minimizer per three bases: 1024 kept
 * minimizers are an overlap region of some 3 kb, which estimated overlaps rarely exceed.
 *
 * Every loop is bounded by a slice size or by the slot count.  What the input's contract excludes (a hash twice in one slice: more
 * shared minimizers than the target slice holds; a table without a free slot) sets OVC_EINTERNAL in the record and fails the call.
 */
#pragma once
#include "dev_common.h"
#include "sketch_kernels.h"

#define OVC_NT 256
#define OVC_LDS_SLICE 1024u   /* longest target slice whose arrays live in LDS (NTL_OVERLAP_LDS_SLICE of the ABI) */
#define OVC_OVER_BLOCKS 64u   /* workgroups (and scratch slabs) of the overflow kernel at most */
#define OVC_SLAB_BYTES_PER_MX 36u /* keys u64[2n] + index u32[2n] + three u32[n] */

/* bits of OvcCut::status (NTL_OVERLAP_* of the ABI) */
#define OVC_CUT 1u
#define OVC_GLOBAL 2u
#define OVC_EINTERNAL 4u
/* bits of OvcPair::signs */
#define OVC_SRC_MINUS 1u
#define OVC_TGT_MINUS 2u

struct OvcPair { uint32_t src, tgt, src_start, src_end, tgt_start, tgt_end, src_len, tgt_len, signs, pad; }; /* ntl_overlap_pair */
struct OvcCut { uint32_t status, n_shared, n_comp, src_cut, tgt_cut, pad; uint64_t hash; };                  /* ntl_overlap_cut */

struct OvcArgs {
    const MxRecord *rec;     /* the kept minimizers */
    const uint32_t *mx_off;  /* [nseq + 1] */
    const OvcPair *pairs;
    uint32_t n_pairs;
    OvcCut *out;             /* [n_pairs] */
    uint32_t *over_list;     /* [n_pairs] pairs left to the overflow kernel */
    uint32_t *info;          /* [0] entries of over_list, [1] their longest target slice, [2] != 0: a record carries OVC_EINTERNAL */
    uint8_t *scratch;        /* overflow kernel: gridDim.x slabs of slab_bytes, each for a target slice of slab_cap minimizers */
    uint64_t slab_bytes;
    uint32_t slab_cap;
};

/* a workgroup's per-pair arrays: `cap` = the target slice's size at least */
struct OvcStore {
    uint64_t *keys;   /* [2 cap] the table's keys */
    uint32_t *idx;    /* [2 cap] the table's values: index in the target slice, NTL_NONE = empty; afterwards the runs' first ranks */
    uint32_t *csrc;   /* [cap] shared minimizer of source rank r: its index in the source slice */
    uint32_t *ctgt;   /* [cap] ... and in the target slice */
    uint32_t *trank;  /* [cap] per target index: shared flag, then the target rank */
};

/* the workgroup's reduction (OVC_NT entries each) */
struct OvcRed { uint64_t *mrl; int64_t *end; uint64_t *hash; uint32_t *rank; };

/* first index in [lo, hi) whose position is >= pos (above: > pos) */
__device__ __forceinline__ uint32_t ovc_bound(const MxRecord *rec, uint32_t lo, uint32_t hi, uint32_t pos, bool above)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t p = rec[mid].pos;
        if (above ? p <= pos : p < pos) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

/* is_valid_pos over a position-ordered list: records [first, first + n) */
__device__ __forceinline__ void ovc_slice(const OvcArgs &A, uint32_t seq, uint32_t start, uint32_t end, uint32_t &first, uint32_t &n)
{
    const uint32_t a = A.mx_off[seq], b = A.mx_off[seq + 1];
    first = ovc_bound(A.rec, a, b, start, false);
    const uint32_t last = ovc_bound(A.rec, first, b, end, true);
    n = last - first;
}

__device__ __forceinline__ uint32_t ovc_home(uint64_t key, uint32_t slots) { return (uint32_t)(((key >> 32) * slots) >> 32); }

/* decimal digits of x (1..20) */
__device__ __forceinline__ uint32_t ovc_digits(uint64_t x)
{
    uint32_t d = 1;
    for (uint64_t p = 10; d < 20u; d++, p *= 10u) /* p = 10^d; the product past 10^19 wraps and is not read */
        if (x < p) break;
    return d;
}

__device__ __forceinline__ uint64_t ovc_pow10(uint32_t e) /* e <= 19 */
{
    uint64_t p = 1;
    for (uint32_t i = 0; i < e; i++) p *= 10u;
    return p;
}

/* str(a) > str(b) for the decimal strings Python makes of two integers, without making them: the longer number is divided down to
   the shorter one's digit count; where the two then agree the shorter is a proper prefix, and the smaller string */
__device__ __forceinline__ bool ovc_str_gt(uint64_t a, uint64_t b)
{
    const uint32_t da = ovc_digits(a), db = ovc_digits(b);
    if (da == db) return a > b;
    if (da > db) return a / ovc_pow10(da - db) >= b;
    return a > b / ovc_pow10(db - da);
}

/* (mapped_region_length, median_length_from_end, mid_mx) of a above that of b, both as sums; rank NTL_NONE: no candidate */
__device__ __forceinline__ bool ovc_better(uint64_t mrl_a, int64_t end_a, uint64_t hash_a, uint32_t rank_a,
                                           uint64_t mrl_b, int64_t end_b, uint64_t hash_b, uint32_t rank_b)
{
    if (rank_a == NTL_NONE) return false;
    if (rank_b == NTL_NONE) return true;
    if (mrl_a != mrl_b) return mrl_a > mrl_b;
    if (end_a != end_b) return end_a > end_b;
    return ovc_str_gt(hash_a, hash_b);
}

__device__ __forceinline__ uint32_t ovc_absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

/* One pair on one workgroup; ns, nt > 0 are the slices' sizes, nt <= the store's cap.  s_tmp: OVC_NT words; s_flag: one word. */
template <bool GLOBAL>
__device__ __forceinline__ void ovc_pair(const OvcArgs &A, uint32_t p, const OvcPair &P, uint32_t sa, uint32_t ns, uint32_t ta, uint32_t nt,
                                         const OvcStore &S, const OvcRed &R, uint32_t *s_tmp, uint32_t *s_flag)
{
    const uint32_t t = threadIdx.x;
    const uint32_t slots = 2u * nt;
    const MxRecord *src = A.rec + sa, *tgt = A.rec + ta;
    if (t == 0) *s_flag = 0u;
    for (uint32_t j = t; j < slots; j += OVC_NT) S.idx[j] = NTL_NONE;
    for (uint32_t j = t; j < nt; j += OVC_NT) S.trank[j] = 0u;
    __syncthreads();
    /* the target slice's table: its keys are distinct, an insert claims the first free slot of its probe sequence */
    for (uint32_t j = t; j < nt; j += OVC_NT) {
        const uint64_t key = tgt[j].hash;
        uint32_t s = ovc_home(key, slots);
        bool placed = false;
        for (uint32_t probe = 0; probe < slots; probe++) {
            if (atomicCAS(&S.idx[s], (uint32_t)NTL_NONE, j) == NTL_NONE) { S.keys[s] = key; placed = true; break; }
            if (++s == slots) s = 0u;
        }
        if (!placed) atomicOr(s_flag, 1u);
    }
    __syncthreads();
    /* shared minimizers in source order */
    uint32_t m = 0;
    for (uint32_t base = 0; base < ns; base += OVC_NT) {
        const uint32_t i = base + t;
        uint32_t j = NTL_NONE;
        if (i < ns) {
            const uint64_t key = src[i].hash;
            uint32_t s = ovc_home(key, slots);
            for (uint32_t probe = 0; probe < slots; probe++) {
                const uint32_t x = S.idx[s];
                if (x == NTL_NONE) break;
                if (S.keys[s] == key) { j = x; break; }
                if (++s == slots) s = 0u;
            }
        }
        uint32_t total;
        const uint32_t r = m + block_excl_scan<OVC_NT>(j != NTL_NONE ? 1u : 0u, s_tmp, total);
        if (j != NTL_NONE) {
            if (r < nt) { S.csrc[r] = i; S.ctgt[r] = j; S.trank[j] = 1u; }
            else atomicOr(s_flag, 1u); /* a hash twice in the source slice */
        }
        m += total;
    }
    if (m > nt) m = nt;
    __syncthreads();
    /* target ranks */
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nt; base += OVC_NT) {
        const uint32_t j = base + t;
        uint32_t total;
        const uint32_t e = carry + block_excl_scan<OVC_NT>(j < nt ? S.trank[j] : 0u, s_tmp, total);
        if (j < nt) S.trank[j] = e;
        carry += total;
    }
    __syncthreads();
    /* runs, each scored by the lane at its tail; the table's index words now hold the runs' first ranks */
    const bool src_minus = (P.signs & OVC_SRC_MINUS) != 0u, tgt_minus = (P.signs & OVC_TGT_MINUS) != 0u;
    uint32_t n_comp = 0;
    uint64_t b_mrl = 0, b_hash = 0;
    int64_t b_end = 0;
    uint32_t b_rank = NTL_NONE;
    for (uint32_t base = 0; base < m; base += OVC_NT) {
        const uint32_t r = base + t;
        const bool in = r < m;
        uint32_t tr = 0, head = 0;
        if (in) {
            tr = S.trank[S.ctgt[r]];
            head = r == 0u || ovc_absdiff(tr, S.trank[S.ctgt[r - 1u]]) != 1u ? 1u : 0u;
        }
        uint32_t total;
        const uint32_t run = n_comp + block_excl_scan<OVC_NT>(head, s_tmp, total) + head - 1u; /* (of a lane that is `in`) */
        if (in && head) S.idx[run] = r;
        __syncthreads();
        if (in && (r == m - 1u || ovc_absdiff(S.trank[S.ctgt[r + 1u]], tr) != 1u)) {
            const uint32_t a = S.idx[run], len = r - a + 1u;
            uint32_t mid = r;
            uint64_t mrl = 2u; /* twice the singleton's 1 */
            if (len > 1u) {
                const MxRecord sa_ = src[S.csrc[a]], sb_ = src[S.csrc[r]];
                mrl = (uint64_t)ovc_absdiff(sa_.pos, sb_.pos) + (uint64_t)ovc_absdiff(tgt[S.ctgt[a]].pos, tgt[S.ctgt[r]].pos);
                mid = ovc_str_gt(sa_.hash, sb_.hash) ? r - len / 2u : a + len / 2u;
            }
            const MxRecord ms = src[S.csrc[mid]];
            const int64_t ps = (int64_t)ms.pos, pt = (int64_t)tgt[S.ctgt[mid]].pos;
            const int64_t end = (src_minus ? -ps : ps - (int64_t)P.src_len) + (tgt_minus ? pt - (int64_t)P.tgt_len : -pt);
            if (ovc_better(mrl, end, ms.hash, mid, b_mrl, b_end, b_hash, b_rank)) { b_mrl = mrl; b_end = end; b_hash = ms.hash; b_rank = mid; }
        }
        n_comp += total;
    }
    R.mrl[t] = b_mrl; R.end[t] = b_end; R.hash[t] = b_hash; R.rank[t] = b_rank;
    __syncthreads();
    for (uint32_t step = OVC_NT / 2u; step; step >>= 1) {
        if (t < step && ovc_better(R.mrl[t + step], R.end[t + step], R.hash[t + step], R.rank[t + step], R.mrl[t], R.end[t], R.hash[t], R.rank[t])) {
            R.mrl[t] = R.mrl[t + step]; R.end[t] = R.end[t + step]; R.hash[t] = R.hash[t + step]; R.rank[t] = R.rank[t + step];
        }
        __syncthreads();
    }
    if (t == 0) {
        const uint32_t best = R.rank[0];
        uint32_t status = (GLOBAL ? OVC_GLOBAL : 0u) | (*s_flag ? OVC_EINTERNAL : 0u);
        uint4 lo = make_uint4(0u, m, n_comp, 0u), hi = make_uint4(0u, 0u, 0u, 0u);
        if (best != NTL_NONE) {
            status |= OVC_CUT;
            lo.w = src[S.csrc[best]].pos;
            hi.x = tgt[S.ctgt[best]].pos;
            hi.z = (uint32_t)R.hash[0]; hi.w = (uint32_t)(R.hash[0] >> 32);
        }
        lo.x = status;
        if (status & OVC_EINTERNAL) atomicOr(&A.info[2], 1u);
        uint4 *o = (uint4 *)&A.out[p];
        o[0] = lo;
        o[1] = hi;
    }
}

/* a pair without a minimizer on one side: no cut */
__device__ __forceinline__ void ovc_none(const OvcArgs &A, uint32_t p)
{
    uint4 *o = (uint4 *)&A.out[p];
    o[0] = make_uint4(0u, 0u, 0u, 0u);
    o[1] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(OVC_NT) void overlap_cut_kernel(OvcArgs A)
{
    __shared__ uint64_t s_keys[2 * OVC_LDS_SLICE];
    __shared__ uint32_t s_idx[2 * OVC_LDS_SLICE];
    __shared__ uint32_t s_csrc[OVC_LDS_SLICE], s_ctgt[OVC_LDS_SLICE], s_trank[OVC_LDS_SLICE];
    __shared__ uint32_t s_tmp[OVC_NT];
    __shared__ uint32_t s_flag;
    static_assert(2 * OVC_LDS_SLICE >= 4 * OVC_NT, "the reduction lies in the key array");
    const uint32_t p = blockIdx.x;
    if (p >= A.n_pairs) return;
    const OvcPair P = A.pairs[p];
    uint32_t sa, ns, ta, nt;
    ovc_slice(A, P.src, P.src_start, P.src_end, sa, ns);
    ovc_slice(A, P.tgt, P.tgt_start, P.tgt_end, ta, nt);
    if (ns == 0u || nt == 0u) { /* uniform */
        if (threadIdx.x == 0) ovc_none(A, p);
        return;
    }
    if (nt > OVC_LDS_SLICE) {
        if (threadIdx.x == 0) {
            A.over_list[atomicAdd(&A.info[0], 1u)] = p;
            atomicMax(&A.info[1], nt);
        }
        return;
    }
    OvcStore S;
    S.keys = s_keys; S.idx = s_idx; S.csrc = s_csrc; S.ctgt = s_ctgt; S.trank = s_trank;
    OvcRed R; /* the table's keys are dead when the reduction starts */
    R.mrl = s_keys; R.end = (int64_t *)(s_keys + OVC_NT); R.hash = s_keys + 2 * OVC_NT; R.rank = (uint32_t *)(s_keys + 3 * OVC_NT);
    ovc_pair<false>(A, p, P, sa, ns, ta, nt, S, R, s_tmp, &s_flag);
}

__global__ __launch_bounds__(OVC_NT) void overlap_cut_overflow_kernel(OvcArgs A)
{
    __shared__ uint64_t s_red[3 * OVC_NT];
    __shared__ uint32_t s_rank[OVC_NT];
    __shared__ uint32_t s_tmp[OVC_NT];
    __shared__ uint32_t s_flag;
    const uint32_t n = A.info[0], cap = A.slab_cap;
    uint8_t *slab = A.scratch + (uint64_t)blockIdx.x * A.slab_bytes;
    OvcStore S;
    S.keys = (uint64_t *)slab;
    S.idx = (uint32_t *)(slab + 16ull * cap);
    S.csrc = S.idx + 2ull * cap; S.ctgt = S.csrc + cap; S.trank = S.ctgt + cap;
    OvcRed R;
    R.mrl = s_red; R.end = (int64_t *)(s_red + OVC_NT); R.hash = s_red + 2 * OVC_NT; R.rank = s_rank;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t p = A.over_list[i];
        const OvcPair P = A.pairs[p];
        uint32_t sa, ns, ta, nt;
        ovc_slice(A, P.src, P.src_start, P.src_end, sa, ns);
        ovc_slice(A, P.tgt, P.tgt_start, P.tgt_end, ta, nt);
        if (ns == 0u || nt == 0u || nt > cap) { /* (the list holds neither) */
            if (threadIdx.x == 0) {
                ovc_none(A, p);
                A.out[p].status = OVC_GLOBAL | OVC_EINTERNAL;
                atomicOr(&A.info[2], 1u);
            }
            continue;
        }
        ovc_pair<true>(A, p, P, sa, ns, ta, nt, S, R, s_tmp, &s_flag);
        __syncthreads(); /* the slab and the reduction are reused by the next pair */
    }
}
