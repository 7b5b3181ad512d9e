/*
 * Text of indexlr's TSV (`indexlr --long --pos [--strand] [--len]`, ntLink:199,223,244,249) made ON THE DEVICE from the 16-byte
 * records of a resident sketch: what ntl_write_indexlr (ntl_io.cpp) makes of the downloaded columns, byte for byte.
 *
 * A line is   name \t [len \t] tok tok ... tok \n   with  tok = H:pos[:S]  (S = + / -), tokens separated by one space; a sequence
 * without a minimizer still has its line, `name \t [len \t] \n`.  The scheme is that of format_kernels.h -- lengths first, offsets by
 * scans, bytes last -- over the sequences [seq_lo, seq_lo + n_seq) of the sketch and their minimizers [mx_lo, mx_lo + n_mx):
 *
 *   sktext_kernel<false>   one lane per minimizer: tok_len = the token and the ONE byte behind it (a space, or the line's newline
 *                          behind the last token: decided when the bytes are written, so that a token's length does not depend on
 *                          its place in the line);
 *                          one lane per sequence: hdr_len = the name, the tab, the length column, and the newline of a line
 *                          without a token.
 *   (scans)                tok_len and hdr_len exclusive-scanned in place with the totals behind them (scan_launch).
 *   sktext_kernel<true>    token j of sequence s starts at hdr_off[s + 1] + tok_off[j], the header of s at
 *                          hdr_off[s] + tok_off[first token of s].  A minimizer finds its sequence by a binary search over
 *                          mx_off (dense and sorted), as fmt_fill_kernel finds a hit's mapping.
 *
 * The bytes and their number come from ONE body each (sktext_token, sktext_header) over a sink that either counts or writes, so
 * the two passes cannot disagree -- what pair_read_body does for count and emit.  Numbers are written back to front by the
 * helpers of format_kernels.h.  Offsets are 32 bits: the host side refuses a range whose bound reaches them.
 */
#pragma once
#include "format_kernels.h"
#include "sketch_kernels.h"

#define SKTEXT_NT 256
#define SKTEXT_TOKEN_MAX 34u /* 20 digits : 10 digits : S and the byte behind the token */
#define SKTEXT_HEADER_EXTRA 13u /* beside the name: the tab, ten digits and their tab, the newline of an empty line */

struct SkTextArgs {
    const MxRecord *recs;    /* the sketch's records */
    const uint32_t *mx_off;  /* [nseq + 1] of the whole sketch */
    const uint64_t *name_off; const char *names; /* device copies of the batch's name table */
    const uint32_t *seq_len; /* the `--len` column (read with with_len only) */
    uint32_t seq_lo, n_seq;  /* the range's first sequence and the number of its sequences */
    uint32_t mx_lo, n_mx;    /* mx_off[seq_lo] and the number of the range's minimizers */
    int with_len, with_strand;
    uint32_t *tok_len, *hdr_len; /* n + 1 entries each: lengths, then (scanned in place) offsets with the total behind them */
    char *text;              /* fill: the text */
};

/* counts the bytes of a piece of text, or writes them at p as well */
template <bool FILL> struct SkSink {
    char *p;
    uint32_t n = 0;
    __device__ __forceinline__ explicit SkSink(char *at) : p(at) {}
    __device__ __forceinline__ void ch(char c) { if (FILL) p[n] = c; n++; }
    __device__ __forceinline__ void u32(uint32_t v) { const uint32_t d = fmt_digits(v); if (FILL) fmt_put_u32(p + n + d, v); n += d; }
    __device__ __forceinline__ void u64(uint64_t v) { const uint32_t d = fmt_digits64(v); if (FILL) fmt_put_u64(p + n + d, v); n += d; }
    __device__ __forceinline__ void bytes(const char *s, uint32_t len)
    {
        if (FILL) for (uint32_t i = 0; i < len; i++) p[n + i] = s[i];
        n += len;
    }
};

/* H:pos[:S] and the byte behind it -> its length (`last` matters to the bytes alone) */
template <bool FILL> __device__ __forceinline__ uint32_t sktext_token(const MxRecord R, int with_strand, bool last, char *p)
{
    SkSink<FILL> o(p);
    o.u64(R.hash); o.ch(':'); o.u32(R.pos);
    if (with_strand) { o.ch(':'); o.ch(R.meta & 1u ? '+' : '-'); }
    o.ch(last ? '\n' : ' ');
    return o.n;
}

/* name \t [len \t] and, for a sequence without a minimizer, the newline -> its length */
template <bool FILL> __device__ __forceinline__ uint32_t sktext_header(const SkTextArgs &A, uint32_t seq, bool empty, char *p)
{
    SkSink<FILL> o(p);
    const uint64_t n0 = A.name_off[seq];
    o.bytes(A.names + n0, (uint32_t)(A.name_off[seq + 1] - n0));
    o.ch('\t');
    if (A.with_len) { o.u32(A.seq_len[seq]); o.ch('\t'); }
    if (empty) o.ch('\n');
    return o.n;
}

/* FILL = false: the lengths.  FILL = true: tok_len / hdr_len hold their exclusive scans. */
template <bool FILL> __global__ __launch_bounds__(SKTEXT_NT) NTL_MAIN_STREAM_SGPRS void sktext_kernel(SkTextArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * SKTEXT_NT + threadIdx.x;
    if (i < A.n_mx) {
        const uint32_t g = A.mx_lo + (uint32_t)i; /* the minimizer's number in the sketch */
        if (!FILL) A.tok_len[i] = sktext_token<false>(A.recs[g], A.with_strand, false, nullptr);
        else {
            /* its sequence: the last one of the range whose first minimizer is <= g (sequences without one share an offset with
               the next: the last of them is the owner) */
            uint32_t lo = 0, hi = A.n_seq;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (A.mx_off[A.seq_lo + mid] <= g) lo = mid; else hi = mid;
            }
            char *p = A.text + (uint64_t)A.hdr_len[lo + 1] + A.tok_len[i];
            sktext_token<true>(A.recs[g], A.with_strand, g + 1 == A.mx_off[A.seq_lo + lo + 1], p);
        }
    }
    if (i < A.n_seq) {
        const uint32_t seq = A.seq_lo + (uint32_t)i;
        const uint32_t m0 = A.mx_off[seq], m1 = A.mx_off[seq + 1];
        if (!FILL) A.hdr_len[i] = sktext_header<false>(A, seq, m0 == m1, nullptr);
        else sktext_header<true>(A, seq, m0 == m1, A.text + (uint64_t)A.hdr_len[i] + A.tok_len[m0 - A.mx_lo]);
    }
}
