/*
 * N-masked copies of resident records (ntl_batch_mask) and ASCII with N back from any batch (ntl_batch_download_n).
 *
 * The reference's gap filler writes, per gap, the WHOLE source scaffold, the WHOLE target scaffold and the WHOLE chosen read to two
 * temporary FASTA files with everything but the scaffold end beside the gap / the read piece between its two cuts replaced by N
 * (print_masked_sequences, bin/ntlink_patch_gaps.py:346-389), and reads them back (map_long_reads, :412-442).  A batch is 2-bit bases
 * plus a table of ACGT runs, so the masked copy of a record is the same bases with the run table clipped to [keep_lo, keep_hi):
 *
 *   nmask_count_kernel   a lane per output record: the source record's runs that intersect the range (two binary searches in its
 *                       slice of the run table) -> cnt, first; their sum, "some record keeps more than one run" and
 *                       "some record is not one whole run" -> stats
 *   (device_scan over cnt -> the output's seq_run_first)
 *   nmask_fill_kernel    a lane per output record: its runs, clipped to the range
 *   nmask_copy_kernel    a wavefront per output record: the packed words of the range, a lane per destination word.  Source and
 *                       destination are not aligned to each other modulo 16 bases: a destination word is funnelled from two source
 *                       words (load_bases16).  The first and the last word of a range are shared with the neighbouring records'
 *                       ranges (atomicOr into the zero-filled stream, as synth_slices_kernel does); words in between are stored.
 *   unpack_runs_kernel  a wavefront per run: its bases as ASCII into a buffer the host filled with 'N'
 *
 * Every loop runs to a count from the run table or the arguments.  Records keep their full length: positions and the --len column
 * stay in scaffold / read coordinates and every sketch and map kernel runs on the result unchanged.
 */
#pragma once
#include "dev_common.h"

#define MASK_NT 256

struct MaskArgs {
    const uint32_t *src_packed;
    const uint64_t *src_seq_base;      /* [n_src+1] */
    const uint32_t *src_seq_run_first; /* [n_src+1] */
    const uint32_t *src_run_start, *src_run_len;
    uint32_t n_src;
    const uint32_t *src_seq, *keep_lo, *keep_hi; /* [n]; checked by the host */
    uint64_t n;
    uint32_t *dst_packed;              /* zero-filled */
    const uint64_t *dst_seq_base;      /* [n+1] */
    uint32_t *cnt;                     /* [n+1]: runs kept per record; scanned into the output's seq_run_first */
    uint32_t *first;                   /* [n]: the first kept run, in the source's table */
    const uint32_t *dst_seq_run_first; /* [n+1] */
    uint32_t *dst_run_start, *dst_run_len;
    unsigned long long *stats;         /* [0] runs kept in all (64 bits: the scan's sum is 32), [1] NMASK_* bits */
};

#define NMASK_MULTI 1ull  /* a record keeps several runs */
#define NMASK_IMPURE 2ull /* a record is not one run from its first base to its last */

/* first run r of [r0, r1) with run_start[r] + run_len[r] > pos (ends ascend); r1 if none */
__device__ __forceinline__ uint32_t nmask_first_end_above(const uint32_t *run_start, const uint32_t *run_len, uint32_t r0, uint32_t r1, uint32_t pos)
{
    for (int it = 0; it < 32 && r0 < r1; it++) {
        const uint32_t mid = r0 + ((r1 - r0) >> 1);
        if ((uint64_t)run_start[mid] + run_len[mid] > pos) r1 = mid; else r0 = mid + 1;
    }
    return r0;
}

/* first run r of [r0, r1) with run_start[r] >= pos; r1 if none */
__device__ __forceinline__ uint32_t nmask_first_start_from(const uint32_t *run_start, uint32_t r0, uint32_t r1, uint32_t pos)
{
    for (int it = 0; it < 32 && r0 < r1; it++) {
        const uint32_t mid = r0 + ((r1 - r0) >> 1);
        if (run_start[mid] >= pos) r1 = mid; else r0 = mid + 1;
    }
    return r0;
}

__global__ __launch_bounds__(MASK_NT) void nmask_count_kernel(MaskArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * MASK_NT + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t s = A.src_seq[i] < A.n_src ? A.src_seq[i] : 0u;
    const uint32_t lo = A.keep_lo[i], hi = A.keep_hi[i];
    const uint32_t r0 = A.src_seq_run_first[s], r1 = A.src_seq_run_first[s + 1];
    uint32_t a = r0, c = 0;
    if (lo < hi && r0 < r1) {
        a = nmask_first_end_above(A.src_run_start, A.src_run_len, r0, r1, lo);
        const uint32_t b = nmask_first_start_from(A.src_run_start, a, r1, hi);
        c = b - a;
    }
    A.cnt[i] = c;
    A.first[i] = a;
    if (c) atomicAdd(&A.stats[0], (unsigned long long)c);
    unsigned long long f = c > 1u ? NMASK_MULTI : 0ull;
    bool whole = false; /* the record is one kept run that the range does not clip: from base 0 to its length */
    if (c == 1u) {
        const uint64_t len = A.dst_seq_base[i + 1] - A.dst_seq_base[i];
        whole = lo == 0 && A.src_run_start[a] == 0 && hi == len && A.src_run_len[a] == len;
    }
    if (!whole) f |= NMASK_IMPURE;
    if (f) atomicOr(&A.stats[1], f);
}

__global__ __launch_bounds__(MASK_NT) void nmask_fill_kernel(MaskArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * MASK_NT + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t lo = A.keep_lo[i], hi = A.keep_hi[i];
    const uint32_t o = A.dst_seq_run_first[i], c = A.dst_seq_run_first[i + 1] - o, a = A.first[i];
    for (uint32_t j = 0; j < c; j++) {
        const uint32_t st = A.src_run_start[a + j], en = st + A.src_run_len[a + j];
        const uint32_t cs = st > lo ? st : lo, ce = en < hi ? en : hi;
        A.dst_run_start[o + j] = cs;
        A.dst_run_len[o + j] = ce - cs;
    }
}

__global__ __launch_bounds__(MASK_NT) void nmask_copy_kernel(MaskArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * (MASK_NT / 64) + (threadIdx.x >> 6);
    if (i >= A.n) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lo = A.keep_lo[i], hi = A.keep_hi[i];
    if (lo >= hi) return;
    const uint32_t s = A.src_seq[i] < A.n_src ? A.src_seq[i] : 0u;
    const uint64_t d0 = A.dst_seq_base[i] + lo, d1 = A.dst_seq_base[i] + hi; /* [d0, d1) of the destination stream */
    const uint64_t s0 = A.src_seq_base[s] + lo;
    const uint64_t w0 = d0 >> 4, nw = ((d1 - 1) >> 4) - w0 + 1;
    for (uint64_t j = lane; j < nw; j += 64) {
        const uint64_t w = w0 + j, g0 = w << 4;
        /* the source position of the word's first base; in front of the range it lies at most 15 bases lower: inside the lead pad
           at the least (s0 >= NTL_LEAD_PAD = 16) */
        const uint64_t sg = g0 >= d0 ? s0 + (g0 - d0) : s0 - (d0 - g0);
        const uint32_t v = load_bases16(A.src_packed, sg);
        const uint32_t a = g0 < d0 ? (uint32_t)(d0 - g0) : 0u;          /* bases [a, b) of the word lie in the range */
        const uint32_t b = g0 + 16 > d1 ? (uint32_t)(d1 - g0) : 16u;
        if (a == 0u && b == 16u) {
            A.dst_packed[w] = v;
        } else {
            const uint32_t below_b = b == 16u ? 0xFFFFFFFFu : (1u << (2u * b)) - 1u;
            const uint32_t m = below_b & ~((1u << (2u * a)) - 1u);
            atomicOr(&A.dst_packed[w], v & m);
        }
    }
}

/* out holds 'N' everywhere; out_off[s] = the place of sequence s's first base in it */
__global__ __launch_bounds__(MASK_NT) void unpack_runs_kernel(const uint32_t *packed, const uint64_t *seq_base, const uint32_t *seq_run_first,
                                                              uint32_t nseq, const uint32_t *run_start, const uint32_t *run_len, uint64_t nruns,
                                                              const uint64_t *out_off, uint8_t *out)
{
    const uint64_t r = (uint64_t)blockIdx.x * (MASK_NT / 64) + (threadIdx.x >> 6);
    if (r >= nruns) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t lo = 0, hi = nseq; /* the sequence s with seq_run_first[s] <= r < seq_run_first[s + 1] */
    for (int it = 0; it < 32 && hi - lo > 1u; it++) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seq_run_first[mid] <= r) lo = mid; else hi = mid;
    }
    const uint32_t st = run_start[r], len = run_len[r];
    const uint64_t gp = seq_base[lo] + st;
    uint8_t *dst = out + out_off[lo] + st;
    const uint32_t lut = 0x54474341u; /* "ACGT" little-endian */
    for (uint64_t c = 16u * lane; c < len; c += 16u * 64u) {
        const uint32_t w = load_bases16(packed, gp + c);
        const uint32_t m = len - c < 16u ? (uint32_t)(len - c) : 16u;
        for (uint32_t j = 0; j < m; j++) dst[c + j] = (uint8_t)(lut >> (8u * ((w >> (2u * j)) & 3u)));
    }
}
