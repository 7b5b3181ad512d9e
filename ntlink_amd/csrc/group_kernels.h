/*
 * Grouped lookup: every read is looked up in the contigs of its own group alone -- the gap filler's re-mapping loop, map_long_reads
 * (bin/ntlink_patch_gaps.py:412-442): per gap one read piece against the minimizer dict of the two scaffold ends around the gap, a hash
 * seen twice among the two dropped (read_btllib_minimizers, :397-410).
 *
 *   group_size_kernel   slots of every group that does not fit the LDS table (0 for one that does) and a 1 per such group: the two
 *                       arrays whose scans give the groups' regions of the global scratch array and the number of large groups.
 *   group_probe_kernel  one workgroup per group at a time, groups taken from a counter: builds the group's table, settles its
 *                       duplicates and looks the group's read minimizers up; leaves Cand and rpos exactly as probe_kernel
 *                       (map_kernels.h) leaves them, for the unchanged map kernels.  No table outlives the kernel.
 *
 * The table is the index's (index_common.h): open addressing, IndexSlot's 16 bytes, index_home with the group's own bit count
 * (the smallest table of at least 1024 slots that is at most half full: 2 n + 2 <= slots, as ntl_index_build sizes its own).  It
 * lives in LDS when it has at most GROUP_LDS_SLOTS slots, otherwise in the group's region of the scratch array.  The insert is
 * index_insert_kernel's rule, order-independent: a compare-and-swap on the key claims the slot, the winner stores the position with a
 * plain store, and winner and later arrivals of the key OR into `meta` -- the winner its contig and strand, the others the duplicate
 * bit -- so that no arrival overwrites what another one writes and no separate bitmap has to be folded in afterwards.
 * Every probe loop counts its steps and stops at the table's slot count with GROUP_ERR_PROBE raised in the result's err word: a
 * table that was sized wrongly is an error (ntl_mapres_wait: NTL_EINTERNAL), never an endless loop.
 */
#pragma once
#include "dev_common.h"
#include "sketch_kernels.h"
#include "index_common.h"
#include "map_kernels.h"

#define GROUP_NT 256          /* lanes per workgroup */
#define GROUP_LDS_SLOTS 2048  /* S: slots of the LDS table, 32 KB (ntl_grouped_info::lds_slots) */
#define GROUP_MIN_BITS 10     /* no table is smaller than 1024 slots (ntl_index_build's minimum) */
#define GROUP_ERR_PROBE 2u    /* bit of MapSums::err: a probe sequence did not end within its table */

static_assert((GROUP_LDS_SLOTS & (GROUP_LDS_SLOTS - 1)) == 0 && GROUP_LDS_SLOTS >= (1 << GROUP_MIN_BITS), "S is a power of two");
static_assert(GROUP_LDS_SLOTS * sizeof(IndexSlot) <= 60 * 1024, "static LDS per workgroup stays below 64 KB");

struct GroupArgs {
    const MxRecord *cmx; const uint32_t *c_off; /* the contig sketch: records, mx_off[n_ctg + 1] */
    const MxRecord *rmx; const uint32_t *r_off; /* the read sketch */
    const uint32_t *cg_off, *rg_off;            /* [n_groups + 1]: first contig / first read of every group */
    uint32_t n_groups;
    const uint32_t *big_off;                    /* [n_groups + 1]: first slot of a large group's region of `scratch` */
    IndexSlot *scratch;
    uint32_t *next;                             /* the group counter, zero before the launch */
    Cand *cand; uint32_t *rpos;                 /* [read minimizers] */
    unsigned long long *nfound; uint32_t *err;  /* the result's device sums (MapSums) */
};

/* bits of the table of a group with n contig minimizers */
__device__ __forceinline__ int group_table_bits(uint32_t n)
{
    int bits = GROUP_MIN_BITS;
    while (((uint64_t)1 << bits) < 2ull * n + 2ull) bits++;
    return bits;
}

/* big[g] = slots of group g's table when it does not fit LDS, else 0; big[n_groups + 1 + g] = 1 for such a group */
__global__ void group_size_kernel(GroupArgs A, uint32_t *big)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= A.n_groups) return;
    const uint32_t n = A.c_off[A.cg_off[g + 1]] - A.c_off[A.cg_off[g]];
    const uint32_t slots = 1u << group_table_bits(n);
    const bool large = slots > GROUP_LDS_SLOTS;
    big[g] = large ? slots : 0u;
    big[A.n_groups + 1 + g] = large ? 1u : 0u;
}

/* One group on one workgroup: contig records [c0, c1), read records [r0, r1), the table in `slots` (LDS = true: the workgroup's LDS
 * array, and every access a DS instruction; false: the group's region of the global scratch array). */
template <bool LDS>
__device__ __forceinline__ void group_one(const GroupArgs &A, IndexSlot *slots, IndexSpecial *special, uint32_t c0, uint32_t c1,
                                          uint32_t r0, uint32_t r1, unsigned long long &found)
{
    const int bits = group_table_bits(c1 - c0);
    const uint32_t nslots = 1u << bits, mask = nslots - 1u;
    for (uint32_t i = threadIdx.x; i < nslots; i += GROUP_NT) { slots[i].key = NTL_INF; slots[i].pos = 0; slots[i].meta = 0; }
    if (threadIdx.x == 0) { special->cnt = 0; special->pos = 0; special->meta = 0; special->pad = 0; }
#ifndef NTL_SIM
    if (!LDS) __threadfence();
#endif
    __syncthreads();

    for (uint32_t i = c0 + threadIdx.x; i < c1; i += GROUP_NT) {
        const MxRecord R = A.cmx[i];
        const uint32_t meta = ((R.meta >> 1) << 2) | ((R.meta & 1u) << 1);
        if (R.hash == NTL_INF) { /* the key that equals the empty marker: beside the table, as IndexSpecial is for the index */
            atomicAdd(&special->cnt, 1u);
            atomicOr(&special->pos, R.pos);
            atomicOr(&special->meta, meta);
            continue;
        }
        uint32_t s = (uint32_t)index_home(R.hash, bits);
        for (uint32_t step = 0;; step++) {
            if (step == nslots) { atomicOr(A.err, GROUP_ERR_PROBE); break; } /* a full table: sized wrongly */
            const unsigned long long old = atomicCAS((unsigned long long *)&slots[s].key, (unsigned long long)NTL_INF,
                                                     (unsigned long long)R.hash);
            if (old == NTL_INF) { slots[s].pos = R.pos; atomicOr(&slots[s].meta, meta); break; } /* first arrival */
            if (old == R.hash) { atomicOr(&slots[s].meta, 1u); break; }                            /* seen before: duplicate */
            s = (s + 1u) & mask;
        }
    }
#ifndef NTL_SIM
    if (!LDS) __threadfence();
#endif
    __syncthreads();

    for (uint32_t i = r0 + threadIdx.x; i < r1; i += GROUP_NT) { /* consecutive lanes, consecutive records */
        const uint64_t key = ntl_stream_load(&A.rmx[i].hash);
        const uint64_t pm = ntl_stream_load((const uint64_t *)&A.rmx[i].pos); /* position | (strand | read << 1) << 32 */
        Cand c;
        c.cpos = 0; c.meta = 0;
        if (key == NTL_INF) {
            if (special->cnt == 1) { c.cpos = special->pos; c.meta = (special->meta & ~1u) | 1u; }
        } else {
            uint32_t s = (uint32_t)index_home(key, bits);
            for (uint32_t step = 0;; step++) {
                if (step == nslots) { atomicOr(A.err, GROUP_ERR_PROBE); break; } /* no empty slot: sized wrongly */
                const IndexSlot e = slots[s];
                if (e.key == NTL_INF) break; /* an empty slot ends the probe sequence */
                if (e.key == key) {
                    if (!(e.meta & 1u)) { c.cpos = e.pos; c.meta = e.meta | 1u; }
                    break;
                }
                s = (s + 1u) & mask;
            }
        }
        /* what probe_kernel leaves: the candidate with the read strand in bit 31 of its meta, the position in the read beside it */
        const uint32_t meta = c.meta | ((uint32_t)(pm >> 32) << 31);
        ntl_stream_store((uint64_t *)&A.cand[i], (uint64_t)c.cpos | ((uint64_t)meta << 32));
        A.rpos[i] = (uint32_t)pm;
        found += c.meta & 1u;
    }
}

/* A resident-size grid; a workgroup takes the next group from the counter while groups are left. */
__global__ __launch_bounds__(GROUP_NT) void group_probe_kernel(GroupArgs A)
{
    __shared__ IndexSlot s_slots[GROUP_LDS_SLOTS];
    __shared__ IndexSpecial s_special;
    __shared__ uint32_t s_g;
    unsigned long long found = 0;
    for (;;) {
        if (threadIdx.x == 0) s_g = atomicAdd(A.next, 1u);
        __syncthreads();
        const uint32_t g = s_g; /* uniform */
        if (g >= A.n_groups) break;
        const uint32_t c0 = A.c_off[A.cg_off[g]], c1 = A.c_off[A.cg_off[g + 1]];
        const uint32_t r0 = A.r_off[A.rg_off[g]], r1 = A.r_off[A.rg_off[g + 1]];
        if (r1 > r0) { /* (a group without read minimizers leaves nothing) */
            if ((1u << group_table_bits(c1 - c0)) > GROUP_LDS_SLOTS)
                group_one<false>(A, A.scratch + A.big_off[g], &s_special, c0, c1, r0, r1, found);
            else
                group_one<true>(A, s_slots, &s_special, c0, c1, r0, r1, found);
        }
        __syncthreads(); /* s_g and the LDS table are written again */
    }
    block_count_add(found, A.nfound);
}
