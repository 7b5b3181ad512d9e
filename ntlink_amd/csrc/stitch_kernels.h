/*
 * The gap filler's output text, assembled on the device (ntl_stitch).
 *
 * print_gap_filled_sequences of the reference (bin/ntlink_patch_gaps.py:533-598) concatenates, per path line, slices of scaffolds
 * (reverse-complemented for a `-` node, the first base lower-cased behind an overlap join), slices of reads (reverse-complemented,
 * lower-cased with --soft_mask) and runs of N.  The records stay on the device as the BYTES they were read as (ntl_ascii: a batch
 * keeps neither case nor IUPAC codes), the host lists the pieces as segments with their 64-bit places in the output, and ONE kernel
 * writes the output:
 *
 *   stitch_kernel   the work is divided by OUTPUT bytes: a workgroup owns a tile of STITCH_TILE bytes, a lane one aligned 16-byte
 *                   chunk of it per round (consecutive lanes, consecutive chunks: 4 KiB per workgroup and round).  Two lanes find
 *                   the tile's first and last segment by a bounded binary search in the segments' output offsets; a lane finds its
 *                   chunk's segment between the two.
 *                     - the chunk lies inside one segment (all of a long scaffold but its two ends): 16 source bytes by two
 *                       unaligned 8-byte loads -- from the mirrored place for a reversed piece, then byte-swapped and complemented
 *                       through a 256-entry table in LDS -- or the fill byte sixteen times; lower-casing is arithmetic on the words
 *                     - the chunk holds a segment boundary: the lane walks the segments of its 16 bytes and gathers them one by one
 *                   Either way the chunk leaves as ONE 16-byte store: every output byte is written once, by one lane, without atomics
 *                   (the buffer is rounded up to 16 bytes: the last chunk's tail is zeros nobody reads).
 *
 * Empty segments never reach the device (the host drops them): the offsets ascend strictly, and a segment's first output byte
 * exists wherever NTL_STITCH_LOWER_FIRST is looked at.  Every loop runs to a count from the arguments.
 *
 * The tile: 256 lanes x 16 bytes x 4 rounds = 16 KiB.  The kernel is a copy -- 16 bytes per lane and access are the widest there
 * are, and a workgroup needs 272 bytes of LDS and few registers, so occupancy is bounded by wavefront slots alone; four rounds give
 * the two searches and the table's load 16 KiB to be spread over, and a 100-Mbp scaffold still makes 6000 workgroups.
 */
#pragma once
#include "dev_common.h"

#define STITCH_NT 256
#define STITCH_ROUNDS 4
#define STITCH_TILE (STITCH_NT * 16 * STITCH_ROUNDS)

/* flags of a device segment: bits 0..2 are NTL_STITCH_REVCOMP / _LOWER / _LOWER_FIRST of the C ABI */
#define STITCH_REVCOMP 1u
#define STITCH_LOWER 2u
#define STITCH_LOWER_FIRST 4u
#define STITCH_FILL 0x80000000u /* no source: the byte in bits 8..15 */

struct StitchSeg {
    uint64_t src; /* device address of the piece's first byte (of the record's byte `lo`, whatever the direction) */
    uint32_t flags, pad;
};

struct StitchArgs {
    const uint64_t *off;  /* [n + 1]: the segments' places in the output, strictly ascending; off[n] == total */
    const StitchSeg *seg; /* [n] */
    const uint8_t *comp;  /* [256]: the reference's complement table (bin/ntlink_patch_gaps.py:50-53) */
    uint64_t n, total;
    uint8_t *out;         /* (total + 15) / 16 * 16 bytes, 16-byte aligned */
};

/* the last s of [lo, hi] with off[s] <= pos; off[lo] <= pos is given */
__device__ __forceinline__ uint64_t stitch_segment_of(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t pos)
{
    for (int it = 0; it < 64 && lo < hi; it++) {
        const uint64_t mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= pos) lo = mid; else hi = mid - 1;
    }
    return lo;
}

/* 'A'..'Z' -> 'a'..'z' in each of the eight bytes, every other byte as it is (Python's .lower() on ASCII) */
__device__ __forceinline__ uint64_t stitch_lower8(uint64_t v)
{
    const uint64_t ones = 0x0101010101010101ull;
    const uint64_t x = v & (0x7Full * ones);
    const uint64_t ge_a = x + (0x80ull - 0x41ull) * ones; /* bit 7 of a byte: its low seven bits are >= 'A' (no carry leaves a byte) */
    const uint64_t gt_z = x + (0x80ull - 0x5Bull) * ones; /* ... are > 'Z' */
    const uint64_t upper = ge_a & ~gt_z & ~v & (0x80ull * ones);
    return v | (upper >> 2);
}

/* the table's entry for each of the eight bytes */
__device__ __forceinline__ uint64_t stitch_comp8(const uint8_t *comp, uint64_t v)
{
    uint64_t r = 0;
    for (int j = 0; j < 8; j++) r |= (uint64_t)comp[(v >> (8 * j)) & 0xFFu] << (8 * j);
    return r;
}

/* output byte `idx` of a segment of `len` bytes */
__device__ __forceinline__ uint32_t stitch_byte(const StitchSeg &sg, uint64_t idx, uint64_t len, const uint8_t *comp)
{
    uint32_t v;
    if (sg.flags & STITCH_FILL) v = (sg.flags >> 8) & 0xFFu;
    else {
        const uint8_t *src = (const uint8_t *)(uintptr_t)sg.src;
        v = sg.flags & STITCH_REVCOMP ? comp[src[len - 1 - idx]] : src[idx];
    }
    if (((sg.flags & STITCH_LOWER) || ((sg.flags & STITCH_LOWER_FIRST) && idx == 0)) && v >= 'A' && v <= 'Z') v |= 0x20u;
    return v;
}

__global__ __launch_bounds__(STITCH_NT) void stitch_kernel(StitchArgs A)
{
    __shared__ uint8_t comp[256];
    __shared__ uint64_t ends[2];
    const uint64_t t0 = (uint64_t)blockIdx.x * STITCH_TILE;
    const uint64_t t1 = A.total - t0 < STITCH_TILE ? A.total : t0 + STITCH_TILE; /* the grid covers the output: t0 < total */
    comp[threadIdx.x] = A.comp[threadIdx.x];
    if (threadIdx.x < 2) ends[threadIdx.x] = stitch_segment_of(A.off, 0, A.n - 1, threadIdx.x ? t1 - 1 : t0);
    __syncthreads();
    const uint64_t s0 = ends[0], s1 = ends[1];
    for (uint32_t r = 0; r < STITCH_ROUNDS; r++) {
        const uint64_t o = t0 + 16u * ((uint64_t)r * STITCH_NT + threadIdx.x);
        if (o >= t1) break;
        uint64_t s = stitch_segment_of(A.off, s0, s1, o);
        uint64_t b = A.off[s], e = A.off[s + 1];
        StitchSeg sg = A.seg[s];
        uint64_t w0 = 0, w1 = 0; /* output bytes o..o+7, o+8..o+15 */
        if (e - o >= 16) {
            const uint64_t idx = o - b;
            if (sg.flags & STITCH_FILL) {
                w0 = w1 = (uint64_t)((sg.flags >> 8) & 0xFFu) * 0x0101010101010101ull;
            } else if (sg.flags & STITCH_REVCOMP) { /* output bytes idx..idx+15 = source bytes len-1-idx down to len-16-idx */
                const uint8_t *p = (const uint8_t *)(uintptr_t)sg.src + ((e - b) - 16 - idx);
                w1 = stitch_comp8(comp, __builtin_bswap64(ntl_load_u64_a1(p)));
                w0 = stitch_comp8(comp, __builtin_bswap64(ntl_load_u64_a1(p + 8)));
            } else {
                const uint8_t *p = (const uint8_t *)(uintptr_t)sg.src + idx;
                w0 = ntl_load_u64_a1(p);
                w1 = ntl_load_u64_a1(p + 8);
            }
            if (sg.flags & STITCH_LOWER) { w0 = stitch_lower8(w0); w1 = stitch_lower8(w1); }
            else if ((sg.flags & STITCH_LOWER_FIRST) && idx == 0) w0 = (w0 & ~0xFFull) | stitch_lower8(w0 & 0xFFull);
        } else {
            for (uint32_t k = 0; k < 16; k++) {
                const uint64_t pos = o + k;
                if (pos >= t1) break;
                for (; pos >= e && s < s1;) { /* at most one step per segment of the tile; pos < off[s1 + 1] */
                    s++;
                    b = e; e = A.off[s + 1];
                    sg = A.seg[s];
                }
                const uint64_t v = stitch_byte(sg, pos - b, e - b, comp);
                if (k < 8) w0 |= v << (8 * k); else w1 |= v << (8 * (k - 8));
            }
        }
        *(uint4 *)(A.out + o) = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
    }
}
