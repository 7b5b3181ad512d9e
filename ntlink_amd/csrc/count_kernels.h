/*
 * Called bases per record of a stitched text (ntl_stitched_base_counts): what `abyss-fac` counts of a FASTA file, taken from the
 * text while it is still on the device.
 *
 * The caller cuts the text into records by ascending offsets (header lines and newlines are just more records, which it ignores);
 * out[i] is the number of bytes of [rec_off[i], rec_off[i + 1]) that are one of ACGTacgt.  ONE kernel reads the text once:
 *
 *   base_count_kernel   the work is divided by BYTES, as in stitch_kernel: a workgroup owns a tile of COUNT_TILE bytes, a lane one
 *                       aligned 16-byte chunk of it per round (consecutive lanes, consecutive chunks).  Two lanes find the records
 *                       of the tile's first and last byte by a bounded binary search in rec_off (stitch_segment_of).
 *                         - a chunk is ONE 16-byte load; its two 64-bit words are compared byte-parallel (case folded by | 0x20,
 *                           then an exact zero test per byte against a, c, g and t) into a mask with bit 7 of every called byte,
 *                           and a popcount of the mask under the chunk's byte range is the chunk's count
 *                         - a lane keeps two sums in registers: for the tile's FIRST record and for its LAST one.  A tile inside
 *                           one record (all of a long scaffold but its ends) only ever adds to the first: no search finds anything
 *                           to do (r0 == r1), no lane walks
 *                         - a chunk that holds record boundaries walks them, one step per record; what falls to a record strictly
 *                           between the tile's first and last -- it lies inside the tile -- goes to its counter by an atomic add
 *                       The two sums are reduced over the wavefront (DPP scan), over the four wavefronts through LDS, and leave as
 *                       one vector atomic add each: a tile inside one record costs one atomic.
 *
 * The first tile starts at rec_off[0] rounded down to 16 and the text is readable up to the next multiple of 16 behind its end
 * (ntl_stitch rounds its buffer up), so every load is aligned and in bounds; bytes outside [rec_off[0], rec_off[n_rec]) are masked
 * out, whatever they are.  Empty records are skipped by the search and stepped over by the walk.  Every loop runs to a count from the
 * arguments.  A tile's sum is at most 16384: 32-bit sums, 64-bit counters.
 */
#pragma once
#include "dev_common.h"
#include "stitch_kernels.h"

#define COUNT_NT 256
#define COUNT_ROUNDS 4
#define COUNT_TILE (COUNT_NT * 16 * COUNT_ROUNDS)

struct CountArgs {
    const uint8_t *text;     /* 16-byte aligned, readable up to (end + 15) / 16 * 16 */
    const uint64_t *rec_off; /* [n_rec + 1], non-decreasing; rec_off[0] == begin, rec_off[n_rec] == end, begin < end */
    uint64_t n_rec, base, begin, end; /* base: begin rounded down to 16 */
    unsigned long long *out; /* [n_rec], zeroed */
};

/* bit 7 of every byte of v that is one of ACGTacgt, every other bit 0.  v | 0x20 maps A and a (and no other byte) to 'a', and so
   on; x is 0 in a byte exactly where (x & 0x7F) + 0x7F | x leaves bit 7 clear, and no carry leaves a byte. */
__device__ __forceinline__ uint64_t count_called8(uint64_t v)
{
    const uint64_t ones = 0x0101010101010101ull, low7 = 0x7Full * ones;
    const uint64_t y = v | (0x20ull * ones);
    const uint64_t xa = y ^ (0x61ull * ones), xc = y ^ (0x63ull * ones), xg = y ^ (0x67ull * ones), xt = y ^ (0x74ull * ones);
    const uint64_t miss = (((xa & low7) + low7) | xa) & (((xc & low7) + low7) | xc) & (((xg & low7) + low7) | xg) & (((xt & low7) + low7) | xt);
    return ~miss & (0x80ull * ones);
}

/* the low n bytes of a word, n >= 8: all of it */
__device__ __forceinline__ uint64_t count_below(uint32_t n) { return n >= 8 ? ~0ull : (1ull << (8 * n)) - 1; }

/* called bytes among bytes [a, b) of a chunk, 0 <= a <= b <= 16; m0, m1: count_called8 of its two words */
__device__ __forceinline__ uint32_t count_range(uint64_t m0, uint64_t m1, uint32_t a, uint32_t b)
{
    const uint64_t k0 = count_below(b) & ~count_below(a);
    const uint64_t k1 = count_below(b > 8 ? b - 8 : 0) & ~count_below(a > 8 ? a - 8 : 0);
    return (uint32_t)__popcll(m0 & k0) + (uint32_t)__popcll(m1 & k1);
}

__global__ __launch_bounds__(COUNT_NT) void base_count_kernel(CountArgs A)
{
    __shared__ uint64_t ends[2];
    __shared__ uint32_t part[2][COUNT_NT / 64];
    const uint64_t c0 = A.base + (uint64_t)blockIdx.x * COUNT_TILE; /* the grid covers [base, end): c0 < end */
    const uint64_t t0 = c0 < A.begin ? A.begin : c0;                /* (the first tile alone) */
    const uint64_t t1 = A.end - c0 < COUNT_TILE ? A.end : c0 + COUNT_TILE;
    if (threadIdx.x < 2) ends[threadIdx.x] = stitch_segment_of(A.rec_off, 0, A.n_rec - 1, threadIdx.x ? t1 - 1 : t0);
    __syncthreads();
    const uint64_t r0 = ends[0], r1 = ends[1]; /* rec_off[r0] <= t0 < rec_off[r0 + 1], rec_off[r1] < t1 <= rec_off[r1 + 1] */
    uint32_t first = 0, last = 0;
    for (uint32_t r = 0; r < COUNT_ROUNDS; r++) {
        const uint64_t o = c0 + 16u * ((uint64_t)r * COUNT_NT + threadIdx.x);
        if (o >= t1) break;
        const uint4 q = *(const uint4 *)(A.text + o);
        const uint64_t m0 = count_called8((uint64_t)q.x | (uint64_t)q.y << 32), m1 = count_called8((uint64_t)q.z | (uint64_t)q.w << 32);
        const uint32_t b = t1 - o < 16 ? (uint32_t)(t1 - o) : 16u;
        uint32_t p = o < t0 ? (uint32_t)(t0 - o) : 0u; /* the chunk's bytes [p, b) are the tile's; p < b */
        uint64_t rec = stitch_segment_of(A.rec_off, r0, r1, o + p);
        for (; p < b && rec <= r1; rec++) { /* at most one step per record of the tile */
            const uint64_t e = A.rec_off[rec + 1]; /* >= o + p */
            const uint32_t pe = e - o < b ? (uint32_t)(e - o) : b;
            const uint32_t n = count_range(m0, m1, p, pe);
            if (rec == r0) first += n;
            else if (rec == r1) last += n;
            else if (n) atomicAdd(&A.out[rec], (unsigned long long)n);
            p = pe;
        }
    }
    first = ntl_wave_incl_scan(first); /* lane 63: the wavefront's sum */
    last = ntl_wave_incl_scan(last);
    if ((threadIdx.x & 63) == 63) { part[0][threadIdx.x >> 6] = first; part[1][threadIdx.x >> 6] = last; }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < COUNT_NT / 64; w++) sum += part[threadIdx.x][w];
        if (sum) atomicAdd(&A.out[threadIdx.x ? r1 : r0], (unsigned long long)sum);
    }
}
