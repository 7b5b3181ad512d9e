/*
 * ntlink_amd.h -- C ABI of the MI355X implementation of the ntLink `pair` hot path.
 *
 * The reference (bcgsc/ntLink v1.3.11) has no FFI for this path: its boundary is two
 * executables joined by a pipe (ntLink:221-225).  Each group of entry points below replaces
 * one of them; INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 *   ntl_batch_*   sequence hand-over                <- btllib SeqReader inside `indexlr`
 *                                                      (ntLink:199,223; id/seq semantics of
 *                                                      bin/read_fasta.py:6-46)
 *   ntl_sketch_*  (k,w) minimizer sketch            <- `indexlr --long --pos --strand [--len]
 *                                                      -k K -w W` (ntLink:199,223) and
 *                                                      btllib.Indexlr(path,k,w,LONG_MODE,t)
 *                                                      (bin/ntlink_patch_gaps.py:417-441)
 *   ntl_overlap_filter  valid-region + per-sequence   <- read_minimizer_line (bin/ntlink_overlap_sequences.py:170-190)
 *                 duplicate filter of the k15 w5 sketch
 *   ntl_overlap_cuts  shared minimizers, their runs   <- merge_overlapping (bin/ntlink_overlap_sequences.py:341-417) with
 *                 and the cut of every adjacent pair     filter_minimizers_position (:304-322), get_dist_from_end (:335-339)
 *   ntl_path_chains  linearize, transitive filter and   <- linearize_graph .. remove_duplicate_paths
 *                 the chains of the path graph            (bin/ntlink_stitch_paths.py:221-365)
 *   ntl_index_*   contig minimizer index            <- NtLink.read_minimizers
 *                                                      (bin/ntlink_pair.py:189-211)
 *   ntl_map_*     per-read lookup, hit filtering,   <- NtLink.find_scaffold_pairs body
 *                 accepted contigs, PAF blocks         (bin/ntlink_pair.py:352-408),
 *                                                      get_accepted_anchor_contigs
 *                                                      (bin/ntlink_utils.py:200-294),
 *                                                      print_paf (bin/ntlink_paf_output.py:103-135)
 *   ntl_map_run_grouped  every read looked up in    <- map_long_reads + read_btllib_minimizers
 *                 the contigs of its own group only    (bin/ntlink_patch_gaps.py:397-442): per gap one read
 *                                                      piece against its two scaffold ends
 *   ntl_mapres_gap_cuts  orientation, consistency,  <- the rest of map_long_reads (bin/ntlink_patch_gaps.py:443-489),
 *                 terminal minimizer and the cuts      find_orientation / check_position_consistency (:113-127),
 *                 of every gap of a grouped result     assign_ctg_cut / assign_read_cut (:291-308),
 *                                                      assess_accepted_anchor_contigs (:492-517)
 *   ntl_fastx_*   FASTA/FASTQ(.gz) records          <- `gzip -cd -f FILES |` + SeqReader
 *                                                      (ntLink:113-117,222-223)
 *   ntl_tsv_*     indexlr TSV -> arrays             <- the split()s of bin/ntlink_pair.py:197-207,355-378
 *   ntl_write_*   indexlr TSV / verbose / PAF text  <- indexlr stdout (ntLink:199,223),
 *                                                      bin/ntlink_pair.py:308-313,382-388,
 *                                                      bin/ntlink_paf_output.py:131-135
 *   ntl_sketch_format  indexlr's TSV from a resident  <- indexlr's printing (ntLink:199,223,244,249)
 *                 sketch, on the device
 *   ntl_tally_*   contig-pair tally                 <- bin/ntlink_pair.py:416-435,315-334,157-239
 *   ntl_liftover  verbose mappings through an AGP   <- bin/ntlink_liftover_mappings.py:61-143 (ntLink_rounds:124-125)
 *   ntl_mapres_liftover  the same on a resident     <- liftover_ctg_mappings, print_adjusted_mappings (:61-121)
 *                 map result, on the device
 *   ntl_mapres_pairs  the per-read part of the tally    <- tally_pairs_from_mappings, calculate_pair_info (bin/ntlink_pair.py:222-239,416-435)
 *                 of a resident map result, on the device
 *
 * Conventions: every call returns 0 on success or a negative NTL_E* code; the message is
 * available from ntl_last_error().  All pointers in signatures are HOST pointers unless the
 * name says otherwise; buffers are caller-owned; counts are obtained first, then filled.
 * Handles are opaque; one context per device; calls on one context are not thread-safe, except
 * ntl_host_alloc / ntl_host_free (a reader thread may take staging buffers while another drives the device)
 * and the host-only groups (ntl_fastx_*, ntl_tsv_*, ntl_write_*, ntl_tally_*: one object per thread).
 * Strands are encoded 1 = '+', 0 = '-'.  Results are in input order (reads, then minimizers in
 * position order), exactly as the reference emits them.
 *
 * Environment (tuning and tests; none is needed): NTL_IO_THREADS (parser threads, default
 * min(cores, 32), or one and a half per core of the process's cgroup CPU quota when that is less), NTL_IO_MIN_CHUNK (bytes per parser thread below which fewer threads are used),
 * NTL_IO_NO_MMAP=1 (stream every input through zlib on one thread), NTL_IO_PREAD=1 (plain files through staged preads
 * instead of a mapping), NTL_IO_NO_LIBDEFLATE=1, NTL_POOL_MAX_BYTES (bound of the cache of device blocks, default half the device memory),
 * NTL_IO_GZ_WHOLE_MAX (compressed bytes up to which a gzip file is inflated in one go, default
 * 1/40 of the physical memory within 1..16 GiB), NTL_IO_TRACE=1 (reader diagnostics on stderr), NTL_SKETCH_C / NTL_SKETCH_NT (k-mers per
 * lane, lanes per strip of the sketch kernel), NTL_SKETCH_FAST=0 (exact 64-bit window pass only), NTL_SKETCH_FORCE_REDO=1
 * (every strip takes the 32-bit passes and the exact pass), NTL_SKETCH_THRESH (0: the block-minima window pass for every
 * window instead of the threshold pass for 71 <= w <= 255; x: x candidates per window instead of 10), NTL_SKETCH_THRESH_DIRECT=1
 * (the threshold pass without staged keys for the large windows too), NTL_EMIT_U=2 (a kernel variant kept for the record; the
 * NTL_SKETCH_LANES experiment's code has left the tree, profiles/HISTORY.md 4.12 is its record), NTL_PIPELINE=0 (one stream per context; default: a second stream for
 * the window stage), NTL_PIPELINE_PRIO (0 no stream priorities, 1 = default: MAIN above the window stream, 2 the reverse),
 * NTL_SIDE_STREAM (1: a third stream for the window stage's give-up passes, beside the next sketch's window kernel; 2: a sketch's
 * preparation on it too; default 0: both stay on the window stream; NTL_SIDE_PRIO=0: that stream at the window stream's priority
 * instead of MAIN's),
 * NTL_SKETCH_CAP_GUESS (records a sketch's arrays hold before its count is known; tests force the second round with it),
 * NTL_SKETCH_TEXT_MAX_BYTES (lowers the bytes one ntl_sketch_format call may make; tests cut small sketches into pieces with it).
 */
#ifndef NTLINK_AMD_H
#define NTLINK_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NTL_OK 0
#define NTL_EINVAL (-1)   /* bad argument */
#define NTL_EDEVICE (-2)  /* no usable gfx950 device / HIP runtime error */
#define NTL_ENOMEM (-3)
#define NTL_EINTERNAL (-4) /* an internal invariant failed (reported, never silently ignored) */
#define NTL_ERANGE (-5)    /* ntl_tally_add: an overhang came out negative (the reference asserts) */
#define NTL_EIO (-6)       /* a file could not be created or written completely; ntl_io_errno() has the errno */

typedef struct ntl_ctx ntl_ctx;
typedef struct ntl_batch ntl_batch;
typedef struct ntl_sketch ntl_sketch;
typedef struct ntl_index ntl_index;
typedef struct ntl_mapres ntl_mapres;

/* ---- context ------------------------------------------------------------------------- */

/* Opens device `device` (a HIP ordinal).  Fails with NTL_EDEVICE if there is no GPU: there is
 * no CPU fallback. */
int ntl_ctx_create(int device, ntl_ctx **out);
void ntl_ctx_destroy(ntl_ctx *ctx);
const char *ntl_last_error(const ntl_ctx *ctx);
/* Human-readable device description ("AMD Instinct MI355X gfx950 256 CUs"). */
const char *ntl_ctx_device_name(const ntl_ctx *ctx);
/* Blocks until all work queued on the context's streams has finished.  Also where the failure of work whose handle was
 * destroyed before it finished is reported (see "Asynchrony" below). */
int ntl_ctx_sync(ntl_ctx *ctx);
/* 1 when the window stage of a sketch runs on its own stream beside the previous batch's emit / map kernels (the default),
 * 0 with NTL_PIPELINE=0 (one stream: what a per-kernel profile wants). */
int ntl_ctx_pipelined(const ntl_ctx *ctx);
/* Turns the second stream off / on again at a quiet point (waits for everything queued first).  NTL_EINVAL when the
 * context was created under NTL_PIPELINE=0. */
int ntl_ctx_set_pipeline(ntl_ctx *ctx, int on);
/* 1 while what follows a sketch's first window kernel -- the passes over the strips it gave up -- is queued on a third stream of the
 * context, beside the next sketch's window kernel: a pipelined context that was created under NTL_SIDE_STREAM=1 (or 2). */
int ntl_ctx_side_stream(const ntl_ctx *ctx);

/* Kernel timing with HIP events on the context's stream.  When enabled, every launch of the
 * named kernel groups is bracketed by events; ntl_prof_get returns the accumulated time and
 * launch count since the last ntl_prof_reset.  Names: "sketch_mask", "sketch_emit", "index",
 * "probe", "map", "compact", "format".  "hipMalloc" (always counted, HOST milliseconds): the misses of the context's cache of
 * device blocks. */
int ntl_prof_enable(ntl_ctx *ctx, int on);
int ntl_prof_reset(ntl_ctx *ctx);
int ntl_prof_get(ntl_ctx *ctx, const char *name, double *total_ms, uint64_t *launches);

/* ---- sequences ------------------------------------------------------------------------ */

/* Hands nseq sequences over: sequence i is the ASCII bytes seqs[offsets[i] .. offsets[i+1]).
 * The bytes are copied to the device as they are and packed there to 2 bits/base plus a table of
 * ACGT runs; the result stays on the device until ntl_batch_destroy and the caller's arrays are
 * free again when the call returns.  Replaces: SeqReader -> NtHash input (ntLink:199,223). */
int ntl_batch_create(ntl_ctx *ctx, const char *seqs, const uint64_t *offsets, uint64_t nseq,
                     ntl_batch **out);
void ntl_batch_destroy(ntl_batch *b);
/* The same from bases that are already in the device's layout -- what ntl_fastx_copy_packed + ntl_fastx_runs produce while
 * they parse: packed[ntl_packed_words(bases)] holds 2 bits per base (A/a 0, C/c 1, G/g 2, T/t 3, anything else 0), sixteen per
 * word, base b of the batch at bit position 2 * (16 + b) (sixteen bases of zero padding in front, 4096 behind); offsets[0] = 0;
 * sequence i has the maximal ACGT/acgt runs seq_run_first[i] .. seq_run_first[i+1], run r = run_len[r] bases from offset
 * run_start[r] of its sequence.  A quarter of the bytes of ntl_batch_create cross PCIe and no pack kernel runs. */
uint64_t ntl_packed_words(uint64_t bases);
int ntl_batch_create_packed(ntl_ctx *ctx, const uint32_t *packed, const uint64_t *offsets, uint64_t nseq,
                            const uint32_t *seq_run_first, const uint32_t *run_start, const uint32_t *run_len, uint64_t nruns,
                            ntl_batch **out);
/* The same from a packed stream whose sequences need not be contiguous -- what the one-pass reader (ntl_fastx_next_span /
 * _parse_span / _copy_span) produces: sequence i = lengths[i] bases from base position positions[i] of the stream (in order,
 * non-overlapping; bit position 2 * (16 + positions[i] + j) for its base j), span_positions = positions the stream spans;
 * packed holds ntl_packed_words(span_positions) words.  The words between sequences are never interpreted. */
int ntl_batch_create_packed_at(ntl_ctx *ctx, const uint32_t *packed, uint64_t span_positions, const uint64_t *positions,
                               const uint32_t *lengths, uint64_t nseq, const uint32_t *seq_run_first, const uint32_t *run_start,
                               const uint32_t *run_len, uint64_t nruns, ntl_batch **out);
uint64_t ntl_batch_nseq(const ntl_batch *b);
uint64_t ntl_batch_bases(const ntl_batch *b);

/* Page-locked host memory for the seqs of ntl_batch_create (one DMA instead of a staged copy);
 * the FASTA/FASTQ reader below can parse straight into it.  Optional: any host pointer works.
 * Blocks of 4 MB and more are anonymous mappings on 2-MB boundaries (transparent huge pages where the host grants them) registered
 * with the runtime -- a fifth of hipHostMalloc's time for the same DMA rate; free them with ntl_host_free only. */
int ntl_host_alloc(ntl_ctx *ctx, uint64_t bytes, void **out);
void ntl_host_free(ntl_ctx *ctx, void *p);

/* ---- synthetic workloads (bench / test harness support; no counterpart in the reference) ---- */

/* BASELINE.json's configurations are synthetic (i.i.d. ACGT genome cut into contigs,
 * ONT/HiFi-like reads with substitution / insertion / deletion errors).  These entry points build such
 * batches directly in HBM, in the layout ntl_batch_create leaves, so that a 3 Gbp assembly and 90
 * Gbases of reads need neither host generation nor PCIe.  All sequences are pure ACGT.
 *   ntl_synth_genome: nseq sequences of len[i] uniform random bases (deterministic in seed).
 *   ntl_synth_slices: sequence i = out_len[i] bases read from source sequence src_seq[i] starting at
 *       src_start[i]; reverse[i] != 0 takes the reverse complement of the slice; sub/ins/del are
 *       per-base event probabilities (0,0,0 = exact copy: contigs).  With errors the slice may consume up
 *       to out_len + out_len/8 + 64 source bases, which must fit the source sequence.
 *   ntl_batch_download: the bases back as ASCII (seqs[offsets[i]..offsets[i+1]), offsets[nseq+1]) --
 *       what the tests hand to the oracle.  Only for pure-ACGT batches: every sequence non-empty and one ACGT run from its
 *       first base to its last, however the batch was made (NTL_EINVAL otherwise; ntl_batch_download_n takes any batch).
 *       ntl_synth_slices asks the same of its source batch. */
int ntl_synth_genome(ntl_ctx *ctx, uint64_t seed, const uint32_t *len, uint64_t nseq, ntl_batch **out);
int ntl_synth_slices(ntl_ctx *ctx, const ntl_batch *src, uint64_t seed, uint64_t n, const uint32_t *src_seq,
                     const uint32_t *src_start, const uint32_t *out_len, const uint8_t *reverse,
                     double sub, double ins, double del, ntl_batch **out);
int ntl_batch_download(const ntl_batch *b, char *seqs, uint64_t *offsets);

/* ---- N-masked copies of resident records (the gap filler's temporary files, without the files) ---- */

/* The reference's gap filler writes per gap the whole source scaffold, the whole target scaffold and the whole chosen read as text
 * with everything but the scaffold end beside the gap / the read piece between its two cuts replaced by N
 * (print_masked_sequences, bin/ntlink_patch_gaps.py:346-389; the reads it keeps for that: get_gap_fill_reads, :264-273) and reads
 * the two files back for the re-mapping.  ntl_batch_mask makes the same records from a resident batch (csrc/mask_kernels.h):
 * record i of *out has the FULL length of record src_seq[i] of src, holds that record's bases in [keep_lo[i], keep_hi[i]) and no
 * valid base outside -- exactly what ntl_batch_create makes of the ASCII record with every byte outside the range replaced by N.
 * Positions and the --len column stay in the source record's coordinates; every sketch and map call takes the result.
 *   - src may hold several runs per record (N, IUPAC codes, lower case); the same record may be named any number of times
 *   - an empty range, or one inside a non-ACGT stretch, gives a record without a run: it sketches to nothing
 *   - NTL_EINVAL with a message: src_seq[i] >= the source's sequences, keep_lo[i] > keep_hi[i], keep_hi[i] > the record's length
 *   - n == 0 gives an empty batch
 * The call WAITS for the device (the run count comes back to the host in the middle of it): the caller's arrays are free when it
 * returns and the batch is complete; src may be destroyed at once.  Event name for ntl_prof_get: "batch_mask".
 *
 * ntl_batch_download_n: ntl_batch_download for ANY batch -- upper-case ASCII with N wherever no run covers a base (lower case and
 * IUPAC codes of the input are not kept by a batch: they come back as upper case and as N). */
int ntl_batch_mask(ntl_ctx *ctx, const ntl_batch *src, uint64_t n, const uint32_t *src_seq, const uint32_t *keep_lo,
                   const uint32_t *keep_hi, ntl_batch **out);
int ntl_batch_download_n(const ntl_batch *b, char *seqs, uint64_t *offsets);

/* ---- resident bytes and the stitch (the gap filler's output sequences) ---------------------- */

/* The reference's gap filler ends by concatenating, per path line, slices of scaffolds, slices of the chosen reads and runs of N
 * into the output FASTA (print_gap_filled_sequences, bin/ntlink_patch_gaps.py:533-598): a `-` node and a read that lies the other way
 * round are reverse-complemented, the base behind an overlap join and (--soft_mask) the read piece are lower-cased.  The output
 * carries the input's bytes -- lower case, N, IUPAC codes -- which a batch does not keep, so the records are resident a second time,
 * as they were read:
 *   ntl_ascii_create: record i = bytes[offsets[i] .. offsets[i+1]), shorter than 2^32 bytes, uploaded as it is.  The caller's
 *       arrays are free when the call returns; page-locked memory (ntl_host_alloc) makes the upload one DMA.
 * ntl_stitch writes the concatenation of n_segs segments, in order (csrc/stitch_kernels.h; the work is divided by output bytes):
 *   - a copy segment {store, rec, lo, hi, flags}: bytes [lo, hi) of record rec of stores[store].  NTL_STITCH_REVCOMP: the piece
 *     reversed, every byte through the reference's table (:50-53: ACGTUNMRWSYKVHDB and their lower case; every other byte as it is).
 *     NTL_STITCH_LOWER: then A-Z -> a-z (Python's .lower() on ASCII).  NTL_STITCH_LOWER_FIRST: the piece's first OUTPUT byte alone; an
 *     empty piece lowers nothing, neither its own nor the next piece's.
 *   - a fill segment {NTL_STITCH_FILL, byte, lo, hi, 0}: hi - lo copies of the byte (runs of N, the newline; header lines come
 *     from a small store of `>id\n` records)
 *   - NTL_EINVAL with a message ("segment i: ..."): a store or a record out of range, lo above hi, hi beyond the record, unknown
 *     flag bits, flags on a fill
 *   - n_segs == 0, or nothing but empty segments, gives an empty result; output offsets are 64-bit
 * ntl_stitch only QUEUES (the segments are copied): stores and arrays may go as soon as it returns.  ntl_stitched_copy waits and
 * copies bytes [lo, hi) of the result, so that a writer can take it in pieces into page-locked memory.  Event name for
 * ntl_prof_get: "stitch" (the kernel), "ascii_upload". */
typedef struct ntl_ascii ntl_ascii;
typedef struct ntl_stitched ntl_stitched;
typedef struct { uint32_t store, rec, lo, hi, flags; } ntl_stitch_seg;
#define NTL_STITCH_FILL 0xFFFFFFFFu
#define NTL_STITCH_REVCOMP 1u
#define NTL_STITCH_LOWER 2u
#define NTL_STITCH_LOWER_FIRST 4u
int ntl_ascii_create(ntl_ctx *ctx, const char *bytes, const uint64_t *offsets, uint64_t nrec, ntl_ascii **out);
void ntl_ascii_destroy(ntl_ascii *a);
uint64_t ntl_ascii_nrec(const ntl_ascii *a);
uint64_t ntl_ascii_bytes(const ntl_ascii *a);
int ntl_stitch(ntl_ctx *ctx, const ntl_ascii *const *stores, uint32_t n_stores, const ntl_stitch_seg *segs, uint64_t n_segs,
               ntl_stitched **out);
uint64_t ntl_stitched_bytes(const ntl_stitched *s);
int ntl_stitched_copy(const ntl_stitched *s, uint64_t lo, uint64_t hi, char *out);
void ntl_stitched_destroy(ntl_stitched *s);

/* Called bases per record of a stitched text, counted on the device (csrc/count_kernels.h; the work is divided by bytes): what
 * `abyss-fac` reports of a FASTA file -- n:500, N50, sum -- needs nothing else of the text.  The caller cuts the text into n_rec
 * records by rec_off[n_rec + 1], non-decreasing, inside the result; header lines and newlines are just more records, which it
 * ignores.  out[i] = the number of bytes of [rec_off[i], rec_off[i + 1]) that are one of ACGTacgt (N, n, U and IUPAC codes are not
 * called bases); an empty record counts 0, and so does every record when n_rec records cover no byte.  n_rec == 0 does nothing.
 * NTL_EINVAL with a message: rec_off descends, or ends beyond the result.  The call WAITS: out is filled and rec_off free when it
 * returns.  Event name for ntl_prof_get: "base_count" (the kernel). */
int ntl_stitched_base_counts(const ntl_stitched *s, const uint64_t *rec_off, uint64_t n_rec, uint64_t *out);

/* ---- sketch ---------------------------------------------------------------------------- */

/* Asynchrony.  ntl_sketch_run[_indexed] and ntl_map_run only QUEUE device work and return; no size comes back to the host
 * inside them.  The handles they return are completed on first use: any accessor that needs a count or a record
 * (ntl_sketch_count / _download / _redo_strips, ntl_mapres_n_* / _download, ntl_index_build on a contig sketch) waits for
 * the device then, and ntl_sketch_wait / ntl_mapres_wait do only that and return the status.  A caller that queues batch
 * i+1 before it asks for the results of batch i lets the window kernels of i+1 run beside the lookup and map kernels of i
 * (the reference's pipe between `indexlr` and `ntlink_pair.py` overlaps the same two stages, ntLink:221-225).  Inputs may be
 * destroyed as soon as the call that took them has returned: the library keeps what it still needs by reference count -- the
 * batch a sketch was made from, the sketch a map result was made from, and the INDEX both were queued against (their kernels
 * read it, and a sketch that overflowed its record array is made again from it when its count is asked for); ntl_index_destroy
 * and the other destroy calls only drop the caller's reference.  Destroying a handle that was never asked for anything is
 * allowed; if its work then fails, the next ntl_ctx_sync reports it.
 * Limits: a context holds 512 page-locked result slots, one per PENDING sketch or map result (queued, not yet completed by an
 * accessor or a wait; handles destroyed while pending count until their work has run).  A call that finds none waits for the
 * oldest destroyed-while-pending handle and otherwise fails with NTL_EDEVICE; the library itself never runs more than eight
 * sketches ahead of the device.  COMPLETED handles hold no slot: any number of them may stay alive. */

/* Computes the (k,w) minimizers of every sequence of the batch on the device; the result stays
 * in device memory.  Replaces `indexlr --long --pos --strand -k K -w W` (ntLink:199,223):
 * ntHash canonical hash for the window minimum, second hash as the emitted value, window over
 * valid k-mers, rightmost minimum on ties. */
int ntl_sketch_run(ntl_ctx *ctx, const ntl_batch *b, int k, int w, ntl_sketch **out);
/* The same sketch made FOR one contig index (read batches of the pair stage): every minimizer is looked up in `ix` while it is
 * emitted, and ntl_map_run(ix, this sketch) skips its own lookup pass over the 16-byte records -- per-read lookup of
 * bin/ntlink_pair.py:364-367 fused into the emitter of `indexlr`.  Minimizers and mappings are those of the two-call form;
 * the index may be destroyed once this call has returned (see "Asynchrony"). */
int ntl_sketch_run_indexed(ntl_ctx *ctx, const ntl_batch *b, int k, int w, const ntl_index *ix, ntl_sketch **out);
/* ... and made ONLY to be mapped against `ix` (what the pair stage does with a read batch, whose minimizers the reference
 * never keeps either: bin/ntlink_pair.py:352-367 reads indexlr's lines off a pipe): the 16-byte records are not written.  A
 * minimizer leaves its candidate and its position in the read, the 12 bytes the map kernels read of it (28 with the records).  ntl_sketch_count / _wait / _nseq and ntl_map_run(ix, this sketch) work; ntl_sketch_download with a record column,
 * ntl_index_build, ntl_overlap_filter and a map against another index answer NTL_EINVAL.  Mappings are those of the other forms. */
int ntl_sketch_run_for_map(ntl_ctx *ctx, const ntl_batch *b, int k, int w, const ntl_index *ix, ntl_sketch **out);
/* 0 for a sketch made by ntl_sketch_run_for_map. */
int ntl_sketch_has_records(const ntl_sketch *s);
void ntl_sketch_destroy(ntl_sketch *s);
/* Waits until the sketch is complete; 0 or the error its completion met. */
int ntl_sketch_wait(const ntl_sketch *s);
uint64_t ntl_sketch_nseq(const ntl_sketch *s);
/* Total number of minimizers. */
uint64_t ntl_sketch_count(const ntl_sketch *s);
/* Diagnostics of the window pass: strips (workgroups) it was cut into, and how many of them the 32-bit pass
 * handed to the exact 64-bit pass (k-mers that share a window and the top 32 hash bits: low-complexity
 * sequence).  The result is the same either way. */
uint64_t ntl_sketch_strips(const ntl_sketch *s);
uint64_t ntl_sketch_redo_strips(const ntl_sketch *s);
/* ... and how many strips the threshold pass (71 <= w <= 255: only k-mers with a small key are looked at) handed to the
 * block-minima pass because one of their windows had no such k-mer (about 0.7 % on random sequence). */
uint64_t ntl_sketch_fallback_strips(const ntl_sketch *s);
/* ... and whether the window passes wrote per-strip minimizer LISTS (1: the windows ntLink runs with, 94 <= w <= 1151, k <= 64) or
 * the bitmask of one bit per base (0: every other window; NTL_SKETCH_LISTS=0; a sketch whose lists ran out of room -- low-complexity
 * sequence throughout -- and was made again).  The result is the same either way. */
int ntl_sketch_from_lists(const ntl_sketch *s);
/* ... and the plan of the window pass that the last round of the sketch carried out, as decided for its (k, w), the number of
 * streams and the tuning knobs -- which kernel ran, on which strips (diagnostics and tests; the result is the same whatever it says).
 * pass: NTL_PASS_*; nt lanes of C k-mers make a strip, which owns NWO windows; big: the two-level form of the block-minima pass (of the
 * list pass behind the wave kernel); direct: the threshold pass without staged keys; wave_*: the four template numbers of
 * sketch_wave_kernel (0 for every other pass); lists as ntl_sketch_from_lists; thresh: keys below it are candidates (0: none). */
enum { NTL_PASS_SMALL = 0, NTL_PASS_EXACT_ONLY = 1, NTL_PASS_BLOCK_MINIMA = 2, NTL_PASS_THRESH = 3, NTL_PASS_WAVE = 4 };
typedef struct ntl_plan_info {
    int32_t pass;
    int32_t nt, C, NWO;
    int32_t big, direct;
    int32_t wave_wavefronts, wave_slots, wave_rounds, wave_kmers; /* wavefronts per workgroup, slots per lane, scan rounds, k-mers per lane */
    int32_t lists;
    uint32_t thresh;
} ntl_plan_info;
int ntl_sketch_plan(const ntl_sketch *s, ntl_plan_info *out);
/* mx_off[nseq+1]: minimizers of sequence i are [mx_off[i], mx_off[i+1]); hash/pos/strand hold
 * ntl_sketch_count() entries (the three fields `indexlr` prints as H:pos:strand). */
int ntl_sketch_download(const ntl_sketch *s, uint64_t *mx_off, uint64_t *hash, uint32_t *pos,
                        uint8_t *strand);
/* Builds a device-resident sketch from host arrays (the text TSV path of the reference:
 * `ntlink_pair.py -m contigs.tsv FILES`, bin/ntlink_pair.py:195-207,355-378). */
int ntl_sketch_from_host(ntl_ctx *ctx, uint64_t nseq, const uint64_t *mx_off, const uint64_t *hash,
                         const uint32_t *pos, const uint8_t *strand, ntl_sketch **out);

/* ---- overlap-stage consumer (k15 w5 sketch) ---------------------------------------------------- */

/* The minimizers the overlap stage keeps per sequence: read_minimizer_line / read_minimizers of
 * bin/ntlink_overlap_sequences.py:145-190 (ntLink:243-251 pipes `indexlr --long --pos -k 15 -w 5` into it).  Sequence i has the
 * valid regions region_start[r] .. region_end[r] (inclusive positions, is_in_valid_region :138-143) for r in
 * region_off[i] .. region_off[i+1]; a sequence without regions (a name that is not in valid_mx_positions) keeps nothing.  Of the
 * minimizers inside a region, every hash that occurs more than once in the sequence is dropped entirely.  The result is a new
 * device-resident sketch with the same sequences and the kept minimizers in their original order (ntl_sketch_download gives
 * the arrays); the input sketch is left alone. */
int ntl_overlap_filter(ntl_ctx *ctx, const ntl_sketch *s, const uint64_t *region_off, const uint32_t *region_start,
                       const uint32_t *region_end, ntl_sketch **out);

/* The cut points of adjacent contigs that overlap: merge_overlapping (bin/ntlink_overlap_sequences.py:341-417) for every pair of a
 * path file in one device pass, on a sketch as ntl_overlap_filter returns it (per sequence the kept minimizers: unique hashes, in
 * position order).  Nothing is changed but `out`; the call waits.
 *
 * ntl_overlap_pair, one per `source gap target` triple that qualifies (:461-468):
 *   src, tgt              the two contigs' sequence numbers in the sketch
 *   *_start, *_end        the pair's valid region on each, both ends inclusive (is_valid_pos :297-301): find_valid_mx_region
 *                         (bin/ntlink_utils.py:189-197) of the source with source=True and of the target with source=False, a
 *                         negative start clamped to 0
 *   src_len, tgt_len      scaffolds[..].length, for get_dist_from_end (:335-339)
 *   signs                 NTL_OVERLAP_SRC_MINUS / NTL_OVERLAP_TGT_MINUS where the node's sign in the path is '-'
 * ntl_overlap_cut, one per pair:
 *   status                NTL_OVERLAP_CUT: a cut was found (merge_overlapping returns True); NTL_OVERLAP_GLOBAL (diagnostics): the
 *                         target slice held more than NTL_OVERLAP_LDS_SLICE minimizers and the pair took the global-scratch path
 *   n_shared              minimizers in both slices (filter_minimizers_position, then ntjoin_utils.filter_minimizers)
 *   n_comp                components of the weight-2 graph (build_graph :246-278, filter_graph_global :288-294): runs of consecutive
 *                         shared minimizers in source order whose target ranks step by one
 *   src_cut, tgt_cut      the chosen mid_mx's position on either contig (:409), for set_scaffold_info; 0 without a cut
 *   hash                  that minimizer (path.mid_mx); 0 without a cut
 * The best component is the maximum of (mapped_region_length, median_length_from_end, mid_mx) with mid_mx compared as the decimal
 * string it is in the reference (:407-408); a component of two or more is walked from the end whose hash is the smaller string
 * (:367-369).  The medians of two integers are compared as sums, in integers.
 * NTL_EINVAL with a message: a sequence number outside the sketch, a region whose start lies behind its end, a NULL array with a
 * non-zero count, a sketch without records, 2^31 pairs or more.  NTL_EINTERNAL: a slice that breaks the sketch's contract. */
#define NTL_OVERLAP_CUT 1u
#define NTL_OVERLAP_GLOBAL 2u
#define NTL_OVERLAP_LDS_SLICE 1024u
#define NTL_OVERLAP_SRC_MINUS 1u
#define NTL_OVERLAP_TGT_MINUS 2u
typedef struct { uint32_t src, tgt, src_start, src_end, tgt_start, tgt_end, src_len, tgt_len, signs, pad; } ntl_overlap_pair;
typedef struct { uint32_t status, n_shared, n_comp, src_cut, tgt_cut, pad; uint64_t hash; } ntl_overlap_cut;
int ntl_overlap_cuts(ntl_ctx *ctx, const ntl_sketch *s, const ntl_overlap_pair *pairs, uint64_t n_pairs, ntl_overlap_cut *out);

/* ---- path chains ----------------------------------------------------------------------- */

/* The graph half of the stitch-paths stage: linearize_graph (bin/ntlink_stitch_paths.py:221-254), is_graph_linear (:256-265),
 * transitive_filter / has_transitive_support (:327-365), find_paths / find_paths_process (:282-300, :314-325) and
 * remove_duplicate_paths (:302-312), on the device (csrc/path_kernels.h).  The reference builds an igraph graph, copies it per
 * filter and takes a subgraph and a shortest path per component.  The call waits once.
 *
 * Vertices are oriented contigs, 2 * contig + (orientation == '-'), so n_vertices is even and the twin of v is v ^ 1.
 *   edges[n_edges]   {src, tgt, d, n, flags}: d the gap, n how many path files gave the edge, NTL_PATH_EDGE_NEW in flags where
 *                    path_id is "new".  Every edge stands beside its twin (tgt ^ 1, src ^ 1) with the same d, n and flags,
 *                    and no (src, tgt) occurs twice.
 *   links[n_links]   {a, b}: the directed edges of the scaffold graph, read in mode NTL_PATH_TRANSITIVE only
 *   mode             NTL_PATH_CONSERVATIVE: the graph as it is (--conservative); NTL_PATH_STITCH: linearize_graph first;
 *                    NTL_PATH_TRANSITIVE: then transitive_filter (--transitive)
 * Out, caller-owned:
 *   chain_off[n_vertices / 2 + 1]  chain i is chain_vertex[chain_off[i] .. chain_off[i + 1]), head to tail; chain_off[n_chains]
 *                                  is counts->n_chain_vertices
 *   chain_vertex[n_vertices]       chains of two or more vertices, in the order of their heads' numbers; of a chain and its twin
 *                                  (reversed, every vertex ^ 1) the one with head <= (tail ^ 1); a chain that is its own twin once
 *   chain_d[n_vertices]            beside every vertex the d of the edge behind it, 0 beside a chain's last
 *   counts                         the two totals, the edges removed by linearize_graph and by transitive_filter, and the
 *                                  components that are cycles (find_paths_process finds no source there: they give no path)
 * Linearize, per vertex and side (:224-249): at a vertex with two or more in-edges (out-edges) one edge stays only if ALL of them
 * are new and the largest n is unique -- every other new edge there goes, edges that are not new always stay; an edge goes if
 * either end says so.  Transitive support of a new edge (s, t) comes from scaffold-graph edges (a, b) with a == s or before it and
 * b == t or behind it on the chain: a != s and b != t is full support, a == s alone source, b == t alone target support, and the
 * edge stays iff it has full support or both of the others.
 * NTL_EINVAL with a message: a vertex beyond n_vertices, an odd n_vertices, an edge twice or without its twin, unknown flags or
 * mode, a graph that is not linear after linearize (the reference's assert), a NULL array with a non-zero count, 2^31 vertices. */
#define NTL_PATH_EDGE_NEW 1u
#define NTL_PATH_CONSERVATIVE 0u
#define NTL_PATH_STITCH 1u
#define NTL_PATH_TRANSITIVE 2u
typedef struct { uint32_t src, tgt; int32_t d; uint32_t n, flags; } ntl_path_edge;
typedef struct { uint32_t a, b; } ntl_path_link;
typedef struct { uint32_t n_chain_vertices, n_chains, removed_linearize, removed_transitive, cycles, reserved[3]; } ntl_path_counts;
int ntl_path_chains(ntl_ctx *ctx, uint32_t n_vertices, const ntl_path_edge *edges, uint64_t n_edges, const ntl_path_link *links,
                    uint64_t n_links, uint32_t mode, uint32_t *chain_off, uint32_t *chain_vertex, int32_t *chain_d,
                    ntl_path_counts *counts);

/* ---- contig index ---------------------------------------------------------------------- */

/* Builds the minimizer -> (contig, position, strand) table from the contig sketch; a hash that
 * occurs more than once anywhere is dropped entirely (bin/ntlink_pair.py:204-209).
 * ctg_len[n_ctg] are the contig lengths (bin/ntlink_utils.py:65-73), n_ctg == sketch nseq. */
int ntl_index_build(ntl_ctx *ctx, const ntl_sketch *contigs, const uint32_t *ctg_len, uint32_t n_ctg,
                    ntl_index **out);
void ntl_index_destroy(ntl_index *ix);
/* Number of minimizers kept (unique hashes). */
uint64_t ntl_index_size(const ntl_index *ix);

/* ---- mapping ---------------------------------------------------------------------------- */

typedef struct {
    int32_t k;             /* -k */
    int32_t z;             /* -z minimum contig length (ntLink passes 1000) */
    double x;              /* -x fudge factor; 0 = compare with the read length only */
    int32_t sensitive;     /* --sensitive */
    int32_t repeat_filter; /* --repeat-filter */
} ntl_map_params;

/* One accepted (read, contig) mapping = one line of <prefix>.verbose_mapping.tsv
 * (bin/ntlink_pair.py:382-388); its hits are hits[hit_off .. hit_off + n_hits) in read order. */
typedef struct {
    uint32_t read, ctg, n_hits, pad;
    uint64_t hit_off;
} ntl_mapping;

/* ctg_pos:ctg_strand_read_pos:read_strand (bin/ntlink_pair.py:308-313) */
typedef struct {
    uint32_t ctg_pos, read_pos;
    uint8_t ctg_strand, read_strand, pad[2];
} ntl_hit;

/* One line of <prefix>.paf (bin/ntlink_paf_output.py:123-135); col 11 = t_end - t_start. */
typedef struct {
    uint32_t read, ctg;
    uint32_t q_start, q_end, t_start, t_end;
    uint32_t n_hits;
    uint32_t strand;
} ntl_paf;

/* Maps every read of the read sketch: index lookup, optional repeat filter, contig length and
 * span filters, run grouping, subsumption, accepted contigs, PAF blocks.  read_len[nreads] is
 * the `--len` column.  Results stay on the device until downloaded. */
int ntl_map_run(ntl_ctx *ctx, const ntl_index *ix, const ntl_sketch *reads, const uint32_t *read_len,
                const ntl_map_params *params, ntl_mapres **out);
void ntl_mapres_destroy(ntl_mapres *r);
/* Waits until the result is complete; 0 or the error its completion met (NTL_EINTERNAL: the reference's assertion that every
 * accepted contig appears once per read, bin/ntlink_utils.py:262-266, failed; or a grouped result's table was sized wrongly). */
int ntl_mapres_wait(const ntl_mapres *r);
uint64_t ntl_mapres_n_mappings(const ntl_mapres *r);
uint64_t ntl_mapres_n_hits(const ntl_mapres *r);
uint64_t ntl_mapres_n_pafs(const ntl_mapres *r);
/* Number of read minimizers found in the index (before any filter): the hit fraction h. */
uint64_t ntl_mapres_n_index_hits(const ntl_mapres *r);
int ntl_mapres_download(const ntl_mapres *r, ntl_mapping *maps, ntl_hit *hits, ntl_paf *pafs);
/* A completed map result made of the caller's records: the counterpart of ntl_sketch_from_host on the map side (no kernel runs, the
 * three arrays are uploaded), so that ntl_mapres_download and ntl_mapres_format can be given records the mapper would not produce.
 *   maps[n_maps]            in result order; read / ctg index the name tables later handed to ntl_mapres_format (not checked here)
 *   hit_slots[n_hit_slots]  the hit array AS THE DEVICE KEEPS IT: mapping m's hits are hit_slots[maps[m].hit_off .. + maps[m].n_hits).
 *                           The regions ascend with the mapping number and do not overlap; slots in front of the first region,
 *                           between two regions and behind the last one are unused (the mapper leaves such slots too).
 *   pafs[n_pafs]            as ntl_mapres_download hands them out
 * n_hits of the result is the sum of maps[].n_hits; ntl_mapres_download returns the dense restatement (hit_off rewritten to the
 * running sum of n_hits, the hits gathered from their regions).  The result is complete when the call returns (nothing pending), it
 * is not grouped (ntl_mapres_grouped_info and ntl_mapres_gap_cuts refuse it with NTL_EINVAL), n_index_hits is 0, and the arrays may
 * go at once.  NTL_EINVAL with a message: a mapping with n_hits == 0, a region that leaves hit_slots, a region that overlaps the one
 * before it or lies in front of it, a NULL array with a non-zero count, 2^32 - 256 or more records in one array. */
int ntl_mapres_from_host(ntl_ctx *ctx, const ntl_mapping *maps, uint64_t n_maps, const ntl_hit *hit_slots, uint64_t n_hit_slots,
                         const ntl_paf *pafs, uint64_t n_pafs, ntl_mapres **out);

/* The liftover of a resident result through an AGP: liftover_ctg_mappings and print_adjusted_mappings of
 * bin/ntlink_liftover_mappings.py:61-121 (ntLink_rounds:122-125) over records instead of lines (csrc/liftover_kernels.h; ntl_liftover
 * below is the host form, file to file).  table[n_ctg] has one entry per contig number of the INPUT result's contig name space.
 * Per mapping (one input line): mode 0 keeps the line for the grouping and drops its hits; otherwise a hit stays iff
 * ctg_start - 1 <= ctg_pos <= ctg_end - k (signed: with k longer than the component none stays), and with adjust = ctg_pos -
 * (ctg_start - 1), offset = scaf_start - 1 its position becomes offset + adjust (mode 2), offset + (ctg_end - ctg_start + 1 - adjust) - k
 * with the contig strand flipped (mode 3), or stays (mode 1).
 * Per read (consecutive mappings with equal .read): runs of consecutive lines with equal new_ctg; a name keeps the index of its FIRST
 * run; a later run of a known name marks every name whose run lies strictly between the two as subsumed (by name: a name may mark
 * itself, two names each other); the lines of subsumed names go, the remaining consecutive lines of one name are a group, whose kept
 * hits are concatenated in order; a group that is not empty and whose contig positions strictly increase or strictly decrease (one
 * hit does) is one output mapping: n_hits the concatenated count, ctg the new_ctg, read unchanged, input order.
 * *out is an ordinary, completed, non-grouped result without PAF records and with n_index_hits = 0; its hits sit in per-mapping
 * regions that ascend with the mapping number, as ntl_mapres_from_host documents.  `in` is completed by the call, left alone, and may be
 * destroyed afterwards.  One host wait.  Event name for ntl_prof_get: "liftover".
 * NTL_EINVAL with a message: a mapping whose ctg >= n_ctg (the reader's 0xFFFFFFFF among them), a mode above 3, an entry of mode 1 to
 * 3 with scaf_start or ctg_start of 0 or ctg_end < ctg_start, k < 1.  NTL_ERANGE: a lifted position does not fit 32 bits (computed in 64
 * bits on the device, reported at the wait).  No partial result in either case.
 * NTL_LIFT_LANE_LINES: a read of at most so many lines is grouped by one lane, a longer one by a wavefront (the result is the same). */
typedef struct {            /* one per contig number of the INPUT result's contig name space */
    uint32_t new_ctg;       /* number in the OUTPUT name space (path id; the contig's own name where it is not in the AGP) */
    uint32_t mode;          /* 0 = not in the AGP (line kept for grouping, every hit dropped)
                               1 = in the AGP, positions left alone (path id == contig id, or orientation neither + nor -)
                               2 = shift (+), 3 = mirror and flip the contig strand (-) */
    uint32_t scaf_start, ctg_start, ctg_end;   /* 1-based inclusive, as in the AGP; ignored for mode 0 */
} ntl_lift_entry;
#define NTL_LIFT_LANE_LINES 16u
int ntl_mapres_liftover(ntl_ctx *ctx, const ntl_mapres *in, const ntl_lift_entry *table, uint32_t n_ctg, int32_t k, ntl_mapres **out);

/* The pair records of a resident result: the per-read part of ntl_tally_add (tally_pairs_from_mappings, calculate_pair_info,
 * calculate_gap_size, normalize_pair of bin/ntlink_pair.py:157-239,416-435) on the device (csrc/pair_kernels.h), so that a result's
 * tally needs neither its mappings nor its hits on the host.  One ntl_pair_rec per pair ntl_tally_add would record, in the order in
 * which it would record them: src / tgt the contig numbers of the normalised pair (smaller name first; equal names swap), src_ori /
 * tgt_ori 1 = '+', gap in 64 bits, anchor 1 iff both mappings have more than one hit, read the mappings' .read.  ntl_tally_add_pairs
 * (below) does the rest -- the dictionary keyed by pair, which depends on the order across reads -- and leaves the tally as
 * ntl_tally_add over the same reads leaves it.
 *   ntl_pairtab   the device's copy of what the rules need of a tally: per contig the rank of its name and its length, plus k and f.
 *                 Taken from the tally (copied: the tally may go), so that rank, k and f have one definition.  A table made on one
 *                 context serves every context of the same device.  ntl_pairtab_create waits.
 *   read_len      [n_reads], indexed by ntl_mapping.read -- or NULL: a read's length is then the largest read_pos among the first and
 *                 last hits of its mappings, the checkpoint rule (bin/ntlink_pair.py:460-488), and n_reads is ignored
 * A read is a run of consecutive mappings with equal .read; a mapping's first and last hit are read from its region, unused slots
 * between regions are allowed (ntl_mapres_from_host), and a result that names a contig twice in one read is handled by key, as on the host.
 * `r` is completed by the call, left alone, and may be destroyed afterwards.  One host wait in ntl_mapres_pairs, one in
 * ntl_pairs_download (out[ntl_pairs_count()]).  The records' array is sized before their number is known, from the mappings and f: at
 * most max(2, f / 2) records per mapping.  Event name for ntl_prof_get: "pairs".
 * NTL_EINVAL with a message: a grouped result, a mapping whose ctg is beyond the table, a .read >= n_reads when read_len is given.
 * NTL_ERANGE: an overhang of an evaluated pair is negative ("Gap distance estimation less than 0", reported at the wait), or the
 * result would make 2^32 - 256 records or more.  No partial result in any of these cases -- ONE difference from the host path: where
 * ntl_tally_add returns NTL_ERANGE the tally has already taken the pairs in front of the failing one; here nothing of that result is
 * added.  The run aborts either way.
 * NTL_PAIR_LANE_MAPS: a read of at most so many mappings is done by one lane, a longer one by a wavefront (the result is the same). */
typedef struct { uint32_t src, tgt; int64_t gap; uint32_t read; uint8_t src_ori, tgt_ori, anchor, pad; } ntl_pair_rec;
typedef struct ntl_tally ntl_tally;
typedef struct ntl_pairtab ntl_pairtab;
typedef struct ntl_pairs ntl_pairs;
#define NTL_PAIR_LANE_MAPS 16u
int ntl_pairtab_create(ntl_ctx *ctx, const ntl_tally *t, ntl_pairtab **out);
void ntl_pairtab_destroy(ntl_pairtab *pt);
int ntl_mapres_pairs(const ntl_mapres *r, const ntl_pairtab *pt, const uint32_t *read_len /* may be NULL */, uint64_t n_reads, ntl_pairs **out);
uint64_t ntl_pairs_count(const ntl_pairs *p);
int ntl_pairs_download(const ntl_pairs *p, ntl_pair_rec *out);
void ntl_pairs_destroy(ntl_pairs *p);

/* Grouped mapping: ntl_index_build + ntl_map_run once per group, on that group's contigs and reads alone, in one device pass -- the
 * gap filler's re-mapping loop (map_long_reads, bin/ntlink_patch_gaps.py:412-442: per gap one read piece against the minimizer dict
 * of the two scaffold ends around it, read_btllib_minimizers :397-410).  Group g = the contigs [ctg_group_off[g], ctg_group_off[g+1])
 * of the contig sketch and the reads [read_group_off[g], read_group_off[g+1]) of the read sketch; both arrays hold n_groups + 1
 * entries, start at 0, do not decrease and end at their sketch's nseq (anything else: NTL_EINVAL); a group may have no contigs, no
 * reads, or neither.  A hash that occurs more than once among ONE group's contig minimizers is dropped for that group; the same hash
 * in two groups is kept in both; a read minimizer is looked up in its own group only.  The result is an ordinary ntl_mapres: read and
 * contig numbers are those of the two sketches (not per group), order is read order, n_index_hits is the sum over the groups, and
 * every ntl_mapres_* call works on it.  ctg_len[contig nseq] (fewer than 2^29 contigs), read_len[read nseq].  Both sketches must hold
 * records (one made by ntl_sketch_run_for_map: NTL_EINVAL).  The call completes the two sketches first (a host wait: their counts
 * size the work); the result is pending like any map result, and both sketches and all arrays may go as soon as the call returns. */
int ntl_map_run_grouped(ntl_ctx *ctx, const ntl_sketch *contigs, const uint32_t *ctg_len, const uint32_t *ctg_group_off,
                        const ntl_sketch *reads, const uint32_t *read_len, const uint32_t *read_group_off, uint32_t n_groups,
                        const ntl_map_params *params, ntl_mapres **out);
/* Diagnostics of a grouped result: a group with n contig minimizers keeps its table (the smallest power of two >= max(1024, 2 n + 2)
 * slots) in the workgroup's LDS when that is at most lds_slots, otherwise in global scratch memory (the result is the same either
 * way).  NTL_EINVAL for an ordinary result. */
typedef struct { uint32_t lds_slots; uint64_t groups_in_lds, groups_in_global; } ntl_grouped_info;
int ntl_mapres_grouped_info(const ntl_mapres *r, ntl_grouped_info *out);

/* The cut points of every gap of a grouped result: what map_long_reads does with the two accepted contigs of a gap
 * (bin/ntlink_patch_gaps.py:443-489) -- find_orientation and check_position_consistency (:113-127), the terminal minimizer of
 * assess_accepted_anchor_contigs (:492-517: the source's last hit when the read-based orientation equals the source's sign, else its
 * first; the target's first when it equals the target's sign, else its last) and assign_read_cut / assign_ctg_cut (:291-308,
 * situations A-D of :276-288) with the k of the re-mapping (args.k).  The result must come from ntl_map_run_grouped with
 * ctg_group_off[g] = 2g and read_group_off[g] = g (gap g = read g, its source contig 2g, its target contig 2g + 1) and n_gaps must be
 * the read sketch's nseq: anything else, or an ordinary result, is NTL_EINVAL.  src_minus[g] / tgt_minus[g]: 1 where the node's sign
 * in the path is '-'.  The result may still be pending: one kernel is queued behind its own, n_gaps records come back and the call
 * waits once; no hit and no mapping is downloaded.  A result whose completion failed returns that error.
 *   status        0: the cuts are valid; otherwise a set of NTL_GAP_* bits and every other field is 0.  The fallback to the old
 *                 anchors (fallback_old_anchor_cuts, :520-530) and --stringent are the caller's, over this word.
 *   *_ctg_pos     the terminal hit's ctg_pos        -> pairs[..].source_ctg_cut / target_ctg_cut
 *   *_read_cut    assign_read_cut of its read_pos   -> pairs[..].source_read_cut / target_read_cut
 *   *_end_cut     assign_ctg_cut of its ctg_pos     -> the scaffold's three_prime_cut / five_prime_cut
 *   ori           bit 0 / bit 1: the read-based orientation of source / target is '+' */
#define NTL_GAP_NOT_TWO 1u           /* len(accepted_anchor_contigs) != 2 (:443) */
#define NTL_GAP_SRC_MIXED_STRANDS 2u /* find_orientation of the source's hits is None */
#define NTL_GAP_TGT_MIXED_STRANDS 4u
#define NTL_GAP_SRC_POSITIONS 8u     /* check_position_consistency of the source's hits is False */
#define NTL_GAP_TGT_POSITIONS 16u
typedef struct { uint32_t status, src_ctg_pos, src_read_cut, src_end_cut, tgt_ctg_pos, tgt_read_cut, tgt_end_cut, ori; } ntl_gap_cut;
int ntl_mapres_gap_cuts(const ntl_mapres *r, const uint8_t *src_minus, const uint8_t *tgt_minus, uint32_t n_gaps, int32_t k, ntl_gap_cut *out);

/* Which read supports which gap, and the cuts it would give: tally_contig_mapping_info (bin/ntlink_patch_gaps.py:149-175),
 * is_valid_supporting_read with calculate_est_gap_size (:208-246) and find_masking_cut_points (:311-342) over one block of
 * <prefix>.verbose_mapping.tsv as ntl_vmap_copy delivers it: read r has the mappings maps[map_off[r] .. map_off[r + 1]) in file order
 * (map_off[0] = 0, non-decreasing, map_off[n_reads] = n_maps), mapping m column 3 as anchors[m], the hits hits[hit_off .. hit_off +
 * n_hits) and its contig's number in the caller's name table (0xFFFFFFFF: not in it, matches no pair; fewer than 2^31 - 1 contigs);
 * ctg_len[n_ctg] the contigs' lengths (sequences[..].length), large_k = args.large_k.
 *
 * The pairs of the path file come as an open-addressing table made by ntl_gap_pair_table: keys[i] = (source node << 32 | target
 * node), node = contig number << 1 | (1 where the sign is '-'), is pair i.  n_slots is a power of two and at least twice the pairs
 * (a table more than half full, or another slot count: NTL_EINVAL); a probe sequence that does not end within the table fails the
 * call with NTL_EINTERNAL instead of hanging.
 *
 * A mapping is valid iff find_orientation gives '+' or '-' and check_position_consistency holds (:113-127); the read's `length` is the
 * read_pos of the last hit of its last valid mapping (:163).  Every combination i < j of a read's valid mappings, in
 * itertools.combinations order, is looked up as (i, j) and then as reverse_complement_pair(i, j), each node with the mapping's own
 * orientation: every pair found is one candidate record, in the order read, combination, direct before reverse complement.
 *   pair, read    the pair's number; the read's number in the block
 *   anchors       int(anchors) of the pair's two contigs, summed (numpy.mean of the two orders as their sum does, :257)
 *   flags         NTL_GAPSEL_VALID: abs(gap_est) <= length (:243); NTL_GAPSEL_NEGATIVE: a < 0 or b < 0, where the reference asserts
 *                 (:222-223); NTL_GAPSEL_VIA_REVCOMP: found as the reverse complement
 *   *_cut         what find_masking_cut_points would write into the pair for this read (assign_ctg_cut / assign_read_cut with large_k)
 * Two valid mappings of one read on the same contig -- a dict overwrite in the reference, never written by `pair` -- fail the call
 * with NTL_EINVAL.  One host wait for the count, one for the records; no hit and no mapping comes back. */
#define NTL_GAPSEL_VALID 1u
#define NTL_GAPSEL_NEGATIVE 2u
#define NTL_GAPSEL_VIA_REVCOMP 4u
typedef struct { uint32_t pair, read, anchors, flags, source_ctg_cut, source_read_cut, target_ctg_cut, target_read_cut; } ntl_gap_cand;
typedef struct ntl_gap_cands ntl_gap_cands;
/* Host only: slot_keys[n_slots] / slot_vals[n_slots] from keys[n_pairs] (distinct, none all ones); NTL_EINVAL unless n_slots is a
 * power of two >= max(2, 2 n_pairs). */
int ntl_gap_pair_table(const uint64_t *keys, uint64_t n_pairs, uint64_t *slot_keys, uint32_t *slot_vals, uint64_t n_slots);
int ntl_gap_select(ntl_ctx *ctx, const uint32_t *map_off, uint32_t n_reads, const ntl_mapping *maps, const uint32_t *anchors,
                   uint64_t n_maps, const ntl_hit *hits, uint64_t n_hits, const uint32_t *ctg_len, uint32_t n_ctg, int32_t large_k,
                   const uint64_t *slot_keys, const uint32_t *slot_vals, uint64_t n_slots, ntl_gap_cands **out);
uint64_t ntl_gap_cands_count(const ntl_gap_cands *s);
int ntl_gap_cands_copy(const ntl_gap_cands *s, ntl_gap_cand *out);
void ntl_gap_cands_destroy(ntl_gap_cands *s);

/* ---- host-side native I/O (no GPU involved) ------------------------------------------------ */

/* FASTA/FASTQ(.gz) reader = `gzip -cd -f FILE | SeqReader` of the reference's pipe
 * (ntLink:113-117,222-223); record semantics of bin/read_fasta.py:6-46.  path "-" = stdin. */
typedef struct ntl_fastx ntl_fastx;
int ntl_fastx_open(const char *path, ntl_fastx **out);
void ntl_fastx_close(ntl_fastx *r);
const char *ntl_fastx_error(const ntl_fastx *r);
/* Collects records until about max_bases bases are held (0 = whole input); *nseq == 0 at the end.
 * Plain regular files are memory-mapped and parsed by several threads (NTL_IO_THREADS, default
 * min(cores, 32)) over byte ranges cut at record boundaries; gzip and stdin go through zlib on one.
 * ntl_fastx_sizes + ntl_fastx_copy gather the batch into caller-allocated arrays (offsets and
 * name_offsets: nseq + 1 entries): sequence i is seqs[offsets[i]..offsets[i+1]), its id
 * names[name_offsets[i]..name_offsets[i+1]).  The pointer accessors return a contiguous copy held
 * by the reader, valid until the next call. */
int ntl_fastx_next(ntl_fastx *r, uint64_t max_bases, uint64_t *nseq);
/* A reader over the records of a plain (uncompressed, regular) file whose FIRST byte lies in [lo, hi) -- hi = 0: to the
 * end -- so that readers opened on [a, b) and [b, c) together see every record once, in order.  NTL_EINVAL for inputs
 * that cannot be cut (gzip, pipes).  ntl_fastx_range reports the bytes [*lo, *hi) the reader really covers (cut at
 * record starts).  The multi-GPU driver gives every rank its own range of the concatenated read files (ntLink:222). */
int ntl_fastx_open_range(const char *path, uint64_t lo, uint64_t hi, ntl_fastx **out);
void ntl_fastx_range(const ntl_fastx *r, uint64_t *lo, uint64_t *hi);
void ntl_fastx_sizes(const ntl_fastx *r, uint64_t *nseq, uint64_t *bases, uint64_t *name_bytes);
int ntl_fastx_copy(const ntl_fastx *r, char *seqs, uint64_t *offsets, char *names, uint64_t *name_offsets);
/* The current batch in the layout of ntl_batch_create_packed instead of ASCII: packed[ntl_packed_words(bases)], offsets and names
 * as above, *nruns = number of ACGT runs; ntl_fastx_runs then fills seq_run_first[nseq + 1], run_start[nruns], run_len[nruns]. */
int ntl_fastx_copy_packed(ntl_fastx *r, uint32_t *packed, uint64_t *offsets, char *names, uint64_t *name_offsets, uint64_t *nruns);
int ntl_fastx_runs(const ntl_fastx *r, uint32_t *seq_run_first, uint32_t *run_start, uint32_t *run_len);
/* One pass instead of two (count, then parse into place): ntl_fastx_next_span cuts the next span of about max_bases bases
 * without reading it (*span_bytes = 0 at the end of the input; *packed_words = words the packed array must hold: every parser
 * thread's range gets room for as many bases as it has bytes -- half as many for FASTQ -- rounded up to whole words);
 * ntl_fastx_parse_span packs the bases into place and collects records, ids and ACGT runs per thread; ntl_fastx_copy_span
 * hands them over (positions[nseq] = first base of every sequence in the packed stream, lengths[nseq], ids, the run table of
 * ntl_fastx_runs, *span_positions for ntl_batch_create_packed_at).  ntl_fastx_parse_span returns NTL_ERANGE when the span cannot
 * be read this way (a range that ends inside a wrapped FASTQ quality section, qualities shorter than their bases): nothing was
 * consumed and ntl_fastx_next reads the same records the two-pass way. */
int ntl_fastx_next_span(ntl_fastx *r, uint64_t max_bases, uint64_t *span_bytes, uint64_t *packed_words);
int ntl_fastx_parse_span(ntl_fastx *r, uint32_t *packed, uint64_t *nseq, uint64_t *bases, uint64_t *name_bytes, uint64_t *nruns);
int ntl_fastx_copy_span(const ntl_fastx *r, uint64_t *positions, uint32_t *lengths, char *names, uint64_t *name_offsets,
                        uint32_t *seq_run_first, uint32_t *run_start, uint32_t *run_len, uint64_t *span_positions);
const char *ntl_fastx_seqs(ntl_fastx *r);
const uint64_t *ntl_fastx_offsets(ntl_fastx *r);
const char *ntl_fastx_names(ntl_fastx *r);
const uint64_t *ntl_fastx_name_offsets(ntl_fastx *r);

/* Text emitters, written to file descriptor fd.  Names are concatenated ids + offsets[n+1].
 * ntl_write_indexlr: `id\t[len\t]H:pos:strand ...` (ntLink:199,223); lengths == NULL omits --len,
 *                    strand == NULL prints `H:pos` (the `--pos`-only form of ntLink:244,249).
 * ntl_write_verbose: <prefix>.verbose_mapping.tsv (bin/ntlink_pair.py:308-313,382-388).
 * ntl_write_paf:     <prefix>.paf (bin/ntlink_paf_output.py:131-135). */
int ntl_write_indexlr(int fd, uint64_t nseq, const char *names, const uint64_t *name_off, const uint32_t *lengths,
                      const uint64_t *mx_off, const uint64_t *hash, const uint32_t *pos, const uint8_t *strand);
int ntl_write_verbose(int fd, const ntl_mapping *maps, uint64_t n_maps, const ntl_hit *hits,
                      const char *read_names, const uint64_t *read_name_off,
                      const char *ctg_names, const uint64_t *ctg_name_off);
int ntl_write_paf(int fd, const ntl_paf *pafs, uint64_t n, const char *read_names, const uint64_t *read_name_off,
                  const uint32_t *read_len, const char *ctg_names, const uint64_t *ctg_name_off, const uint32_t *ctg_len);

/* indexlr TSV parser: the text input of operator B2 (`id\t[len\t]H:pos:strand ...`, split the way
 * bin/ntlink_pair.py:197-207,355-378 split it), several threads over blocks of whole lines.  path "-"
 * = stdin.  ntl_tsv_next reads about max_bytes of text (0 = all of it) and counts; ntl_tsv_copy
 * fills caller-allocated arrays (name_off / mx_off: nrec + 1 entries, lengths may be NULL): record i
 * has the id names[name_off[i]..name_off[i+1]) and the minimizers mx_off[i]..mx_off[i+1]; strand 1 = '+'.
 * A malformed token fails the call (the reference raises ValueError there).  The arrays are what
 * ntl_sketch_from_host takes.  with_len is a flag word: bit 0 = the `--len` column is present, bit 1 = the tokens are
 * `H:pos` (indexlr --pos without --strand, the overlap stage's input, ntLink:244,249; strand[] is then filled with 1). */
typedef struct ntl_tsv ntl_tsv;
int ntl_tsv_open(const char *path, int with_len, ntl_tsv **out);
void ntl_tsv_close(ntl_tsv *r);
const char *ntl_tsv_error(const ntl_tsv *r);
int ntl_tsv_next(ntl_tsv *r, uint64_t max_bytes, uint64_t *nrec);
void ntl_tsv_sizes(const ntl_tsv *r, uint64_t *nrec, uint64_t *nmx, uint64_t *name_bytes);
int ntl_tsv_copy(const ntl_tsv *r, char *names, uint64_t *name_off, uint32_t *lengths, uint64_t *mx_off,
                 uint64_t *hash, uint32_t *pos, uint8_t *strand);

/* Reader of <prefix>.verbose_mapping.tsv for the gap filler: the loop of read_verbose_mappings with the split()s of
 * tally_contig_mapping_info and ntlink_utils.parse_minimizers (bin/ntlink_patch_gaps.py:178-198,153-154) -- lines
 * `read\tcontig\tanchors\tctgpos:ctgstrand_readpos:readstrand ...`, several threads over blocks of whole READS: consecutive lines with
 * the same first column stay in one block (one read, as in the reference; the same id again further on is another read).
 * ntl_vmap_open takes the contig name table (name i = ctg_names[ctg_name_off[i] .. ctg_name_off[i + 1]), copied).  ntl_vmap_next reads
 * about max_bytes of text (0 = all of it; more where one read's lines need it) and counts; *n_reads == 0 at the end.  ntl_vmap_copy
 * fills caller-allocated arrays: read r has the id names[name_off[r] .. name_off[r + 1]) and the lines map_off[r] .. map_off[r + 1]
 * (name_off / map_off: n_reads + 1 entries); line m is maps[m] -- read = r, ctg = the contig's number in the table or 0xFFFFFFFF for a
 * name that is not in it, n_hits = its tokens, hit_off dense -- with column 3 as written in anchors[m] (the reference scores with
 * int(anchors), not with the token count) and the tokens in hits[].  What ntl_gap_select takes.
 * A line that is not four tab-separated fields, a token that is not int:+-_int:+-, column 3 not a number, or a number above
 * 2^32 - 1 fails ntl_vmap_next with NTL_EINVAL and "line N: ..." (N counts from 1 over the whole file) in ntl_vmap_error: never a
 * partial block.  The checkpoint and liftover readers are not this one. */
typedef struct ntl_vmap ntl_vmap;
int ntl_vmap_open(const char *path, const char *ctg_names, const uint64_t *ctg_name_off, uint64_t n_ctg, ntl_vmap **out);
void ntl_vmap_close(ntl_vmap *r);
const char *ntl_vmap_error(const ntl_vmap *r);
int ntl_vmap_next(ntl_vmap *r, uint64_t max_bytes, uint64_t *n_reads);
void ntl_vmap_sizes(const ntl_vmap *r, uint64_t *n_reads, uint64_t *n_maps, uint64_t *n_hits, uint64_t *name_bytes);
int ntl_vmap_copy(const ntl_vmap *r, char *names, uint64_t *name_off, uint32_t *map_off, ntl_mapping *maps, uint32_t *anchors,
                  ntl_hit *hits);

/* ---- the text of the mapping outputs, made on the device ------------------------------------
 * Replaces the formatting loops of bin/ntlink_pair.py:308-313,382-388 (<prefix>.verbose_mapping.tsv) and
 * bin/ntlink_paf_output.py:131-135 (<prefix>.paf): the lines are laid out and written by kernels from the dense records of a map
 * result and two name tables that live on the device; what crosses PCIe is the text itself, the mappings, and -- all the pair tally
 * needs of the hits (bin/ntlink_pair.py:394-406) -- the first and the last hit of every mapping.  The bytes are those of
 * ntl_write_verbose / ntl_write_paf on the same records. */
typedef struct ntl_names ntl_names;
typedef struct ntl_text ntl_text;
/* Name i is names[off[i] .. off[i+1]); len (may be NULL) the sequences' lengths: both tables of ntl_mapres_format need them
 * (PAF columns 2 and 7).  The arrays are copied; they are the caller's again when the call returns. */
int ntl_names_create(ntl_ctx *ctx, const char *names, const uint64_t *off, const uint32_t *len, uint64_t n, ntl_names **out);
void ntl_names_destroy(ntl_names *t);
/* Completes the result (waits for it), then formats: verbose != 0 the lines of .verbose_mapping.tsv, paf != 0 those of .paf.
 * One more host wait inside (the byte totals size the text arrays).  NTL_ERANGE for more than 4 GB of text in one batch.
 * The text keeps what it needs: the result may be destroyed once this call has returned. */
int ntl_mapres_format(const ntl_mapres *r, const ntl_names *reads, const ntl_names *contigs, int verbose, int paf, ntl_text **out);
void ntl_text_sizes(const ntl_text *t, uint64_t *verbose_bytes, uint64_t *paf_bytes, uint64_t *n_mappings);
/* Any destination may be NULL.  ends: 2 * n_mappings hits, {first, last} per mapping (ntl_tally_add_ends). */
int ntl_text_download(const ntl_text *t, char *verbose, char *paf, ntl_mapping *maps, ntl_hit *ends);
void ntl_text_destroy(ntl_text *t);
/* n bytes at the end of fd (O_APPEND or not: the position is taken once), written by the I/O worker pool in parallel pieces. */
int ntl_write_blob(int fd, const char *p, uint64_t n);

/* ---- indexlr's TSV, made on the device ---------------------------------------------------------
 * Replaces indexlr's printing (`indexlr --long --pos --strand [--len]`, ntLink:199,223; the `H:pos` form of the overlap stage,
 * `indexlr --long --pos -k 15 -w 5`, ntLink:244,249): the lines `id\t[len\t]H:pos[:strand] ...` are laid out and written by kernels
 * (csrc/sketch_text_kernels.h) from the records of a resident sketch and a name table that lives on the device; what crosses PCIe is
 * the text itself.  The bytes are those of ntl_write_indexlr on the sketch's downloaded columns; a sequence without a minimizer has
 * its line `id\t[len\t]\n` there too.
 *
 * ntl_sketch_format completes the sketch (waits for it), then formats the lines of the sequences [seq_lo, seq_hi): name i of `names`
 * and its length belong to sequence i of the sketch.  flags: NTL_SKETCH_TEXT_LEN the `--len` column, NTL_SKETCH_TEXT_STRAND the
 * `--strand` column (clear it for `H:pos`).  One host wait inside, for the byte total that sizes the text; the first call on a
 * sketch also fetches its nseq + 1 offsets once, since a range's minimizers size the work.  The text keeps what it needs: sketch
 * and names may be destroyed once the call has returned.  Event name for ntl_prof_get: "sketch_text".
 * Offsets inside one text are 32 bits, so the CALLER cuts a sketch into ranges: a range is taken iff ntl_sketch_text_bound(names,
 * its sequences, its minimizers) -- 34 bytes per minimizer, the longest name + 13 per sequence -- is below ntl_sketch_text_limit()
 * (2^32 - 256, or NTL_SKETCH_TEXT_MAX_BYTES where that is less: a test hook).  A single sequence above the limit is refused, not split.
 *   NTL_EINVAL with a message: a sketch without records (ntl_sketch_has_records() == 0), a name table with fewer names than the
 *   sketch has sequences or on another device, NTL_SKETCH_TEXT_LEN with a table made without lengths, seq_lo > seq_hi, seq_hi beyond
 *   the sketch, unknown flag bits.  NTL_ERANGE with a message: the range's bound reaches the limit; nothing is queued, nothing written.
 * A text offers its byte count, a download into caller memory (waits) and a destroy -- a handle of its own and not an ntl_text, whose
 * sizes and download speak of a map result's two files, its mappings and its hit ends. */
typedef struct ntl_sktext ntl_sktext;
#define NTL_SKETCH_TEXT_LEN 1
#define NTL_SKETCH_TEXT_STRAND 2
int ntl_sketch_format(const ntl_sketch *s, const ntl_names *names, int flags, uint64_t seq_lo, uint64_t seq_hi, ntl_sktext **out);
uint64_t ntl_sketch_text_limit(void);
uint64_t ntl_sketch_text_bound(const ntl_names *names, uint64_t n_seq, uint64_t n_mx);
uint64_t ntl_sktext_bytes(const ntl_sktext *t);
int ntl_sktext_download(const ntl_sktext *t, char *out);
void ntl_sktext_destroy(ntl_sktext *t);

/* ---- host-side pair tally (no GPU involved) ------------------------------------------------- */

/* The contig-pair bookkeeping of bin/ntlink_pair.py (tally_pairs_from_mappings :416-435, add_pair
 * :315-334, calculate_pair_info :222-239, calculate_gap_size :157-187, normalize_pair :213-219)
 * over the records of ntl_map_run.  Pairs are keyed by contig NAME (byte order decides which
 * contig comes first); f = the -f chain-length threshold.  ntl_tally_add takes one batch of reads
 * in order (read_len indexed by ntl_mapping.read) and returns NTL_ERANGE where the reference
 * raises "Gap distance estimation less than 0".  ntl_tally_export lists every pair in order of
 * first appearance: contig indices, orientations (1 = '+'), anchor count and
 * gaps[gap_off[i] .. gap_off[i+1]) in read order (arrays sized from npairs / ngaps).  (ntl_tally is declared with ntl_mapres_pairs.) */
int ntl_tally_create(const char *ctg_names, const uint64_t *ctg_name_off, const uint32_t *ctg_len, uint64_t n_ctg,
                     int k, int f, ntl_tally **out);
void ntl_tally_destroy(ntl_tally *t);
int ntl_tally_add(ntl_tally *t, const ntl_mapping *maps, uint64_t n_maps, const ntl_hit *hits, const uint32_t *read_len);
/* The same from the first and last hit of every mapping alone (ends[2 i], ends[2 i + 1]: ntl_text_download). */
int ntl_tally_add_ends(ntl_tally *t, const ntl_mapping *maps, uint64_t n_maps, const ntl_hit *ends, const uint32_t *read_len);
/* The same from the records ntl_mapres_pairs made of the mappings on the device, in their order: a new pair on first sight, the gap
 * pushed, the anchor added.  After it the tally is what ntl_tally_add over the same reads leaves (ntl_tally_export gives equal arrays).
 * NTL_EINVAL, with nothing added, for a contig number beyond the tally or an orientation above 1. */
int ntl_tally_add_pairs(ntl_tally *t, const ntl_pair_rec *recs, uint64_t n);
uint64_t ntl_tally_npairs(const ntl_tally *t);
uint64_t ntl_tally_ngaps(const ntl_tally *t);
int ntl_tally_export(const ntl_tally *t, uint32_t *src, uint8_t *src_ori, uint32_t *tgt, uint8_t *tgt_ori,
                     uint32_t *anchor, uint64_t *gap_off, int64_t *gaps);
/* Appends an export of ANOTHER tally over the same contigs that covers later reads (pairs first seen there go behind the
 * known ones, gaps behind the gaps of the same pair, anchors add up): what one tally would hold after both read ranges.
 * The multi-GPU driver tallies per rank and merges in rank order on rank 0. */
int ntl_tally_merge(ntl_tally *t, uint64_t npairs, const uint32_t *src, const uint8_t *src_ori, const uint32_t *tgt,
                    const uint8_t *tgt_ori, const uint32_t *anchor, const uint64_t *gap_off, const int64_t *gaps);

/* The two small files behind the tally: <prefix>.pairs.tsv (write_pairs, bin/ntlink_pair.py:490-496; pairs_path may be NULL) and
 * <prefix>.n<n>.scaffold.dot (build_scaffold_graph :263-305, filter_graph_global :498-506 with min_n = n, print_directed_graph
 * :133-155; dot_path may be NULL) from the pairs that pass filter_pairs_distances (:247-255) and filter_weak_anchor_pairs
 * (:241-244, anchor >= a).  *n_kept (may be NULL): the pairs that passed.  Each file is written beside its place and renamed when it
 * is complete (the reference leaves no partial output behind, bin/ntlink_pair.py:608-613); NTL_EIO when a file cannot be created,
 * written or closed, with the errno in ntl_io_errno(). */
int ntl_tally_write(const ntl_tally *t, int a, int min_n, const char *pairs_path, const char *dot_path, uint64_t *n_kept);
/* errno of the calling thread's last call that returned NTL_EIO (0: none). */
int ntl_io_errno(void);

/* ---- liftover of the verbose mappings, file to file (no GPU involved; ntl_mapres_liftover is the device form) ---- */

/* <prefix>.verbose_mapping.tsv moved to the coordinates of the scaffolds an AGP describes, file to file: the work of
 * bin/ntlink_liftover_mappings.py (liftover_ctg_mappings :61-87, print_adjusted_mappings :89-121, liftover_mappings
 * :125-143; called between rounds, ntLink_rounds:124-125).  The AGP's sequence lines (component type not N / P, read_agp
 * :39-50) come as arrays, one entry per contig id (the last line of an id wins, as in the reference's dict): contig id,
 * path id, scaf_start, ctg_start, ctg_end (1-based, inclusive) and the orientation byte.  Per line: a contig that is not in
 * the AGP keeps its name and loses its mappings; mappings outside [ctg_start-1, ctg_end-k] are dropped; `+` / `-`
 * components of a path with another name are shifted / mirrored (strand flipped).  Per read (consecutive lines with one
 * read id): lines are grouped by path id, paths strictly between two occurrences of a path's first run and a later run
 * are subsumed, the surviving lines of a path are concatenated and printed when their contig positions are strictly
 * monotonic.  A malformed line fails the call (the reference raises) and removes the output file.  lines_in / lines_out
 * may be NULL. */
int ntl_liftover(const char *mappings_path, const char *out_path, int k, uint64_t n_agp, const char *ctg_ids,
                 const uint64_t *ctg_id_off, const char *path_ids, const uint64_t *path_id_off, const int64_t *scaf_start,
                 const int64_t *ctg_start, const int64_t *ctg_end, const char *orientation, uint64_t *lines_in,
                 uint64_t *lines_out);

#ifdef __cplusplus
}
#endif
#endif
