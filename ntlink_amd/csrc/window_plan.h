/*
 * The plan of a sketch's window pass: what window_plan() (ntl_hip.hip) decides once per sketch, before anything is allocated or
 * launched, and sketch_enqueue()'s stages carry out: launch_window_pass() in sketch_window_stage(), and sketch_emit_stage() with
 * emit_grid() and emit_launch().
 */
#pragma once
#include "sketch2_kernels.h"

/*
 * Which window pass a sketch runs with no knob set (DESIGN.md 4.1 holds the same table):
 *
 *   2 <= w <= 15, any k                sketch_small_kernel<W>                                                     (SMALL)
 *   w = 1; w > 1151 (w <= 4063);
 *   k > 256 (w = 1 or w >= 16)         sketch_mask_kernel<1 / 16> alone (EXACT_ONLY; <4> and <1> for 2 <= w <= 15 only by knob)
 *   below, k <= 256:
 *   16 <= w < 64                       sketch_fast_kernel<128, R0, true>                                          (BLOCK_MINIMA, big)
 *   64 <= w <= 70                      sketch_fast_kernel<256, R0, false>                                         (BLOCK_MINIMA)
 *   71 <= w <= 93, and
 *   94 <= w <= 120 when k > 64         sketch_thresh_kernel<256, true> + sketch_fast_list_kernel<256, R0>         (THRESH, direct)
 *   121 <= w <= 255 when k > 64        sketch_thresh_kernel<256, false> + sketch_fast_list_kernel<256, R0>        (THRESH)
 *   256 <= w <= 1151 when k > 64       sketch_fast_kernel<256, R0, true>                                          (BLOCK_MINIMA, big)
 *   94 <= w <= 1151, k <= 64           sketch_wave_kernel + sketch_fast_list_kernel<256, R0, w > 255>, strip lists (WAVE; big: w > 255):
 *       94 <= w <= 136                     <4, 19, 8> beside the other stream's kernels, <8, 19, 8> alone
 *       137 <= w <= 234                    <8, 15, 6>
 *       235 <= w <= 1151                   <8, 11, 4>  (by knob, NTL_SKETCH_STRIP=8192: <8, 19, 7, 128> on strips of 8192 ordinals)
 *
 * (w <= 1151: a + 2 <= SK2_PAD blocks right of a window's first, a = (w - 16) / 16.)  tests/test_window_plan.py states the same table
 * a third time, reads it back from sketches (ntl_sketch_plan) on both sides of every boundary, and must change with it.
 * Every 32-bit pass is followed by the exact pass over the strips it flagged.  A sketch has one strip length, nt lanes of 16 k-mers:
 * 4096 ordinals (2048 for w < 64) unless that knob is set, and every pass behind the wave kernel is instantiated for it
 * (sketch_fast_list_kernel<512, ..>, sketch_mask_kernel<16, 512, ..>).  The w boundaries above 70 are those of the candidates
 * 4096 k-mers are expected to hold, 4096 T / 2^32 = 40960 / w at the default ten candidates per window, against:
 */
static const double WP_FIT_THRESH = 580.0; /* above: no threshold (sketch_thresh_kernel<.., DIRECT>'s list of 680 with room for the spread) */
static const double WP_FIT_WAVE = 440.0;   /* above: not sketch_wave_kernel (its largest shape's list: 8 rounds of 64) */
static const double WP_FIT_STAGED = 340.0; /* above: sketch_thresh_kernel without staged keys (402 entries beside them) */
static const double WP_FIT_15_6 = 300.0;   /* above: the <.., 19, 8> shapes, and the emit grid beside these DENSE windows takes four workgroups per CU */
static const double WP_FIT_11_4 = 175.0;   /* above: <8, 15, 6> */

enum WindowPass { WP_SMALL, WP_EXACT_ONLY, /* the 32-bit passes, each with the exact pass over what it flags: */ WP_BLOCK_MINIMA, WP_THRESH, WP_WAVE };
/* sketch_wave_kernel<wavefronts per workgroup, staging slots per lane, scan rounds, k-mers per lane = 64>: the slots hold a lane's 64 p
   candidates + 4.5 sigma, the list (64 per round) a strip's 4096 p + 4 sigma; what does not fit is given up.  <8, 19, 7, 128>: a lane
   stages 5.12 candidates on average at w = 250 and P(Poisson(5.12) > 19) = 5 10^-7, a strip in 3 10^-5 is given up for it (17 slots:
   5 10^-4; the 4096 shape's eleven: 10^-3); the list holds 440 for a mean of 328 (sigma 18).  The first WS_DEFAULTS are some (k, w)'s default */
enum WaveShape { WS_8_11_4, WS_8_15_6, WS_8_19_8, WS_4_19_8, WS_8_19_7_L128, WS_DEFAULTS, WS_4_11_4 = WS_DEFAULTS, WS_16_11_4 };

struct WindowPlan {
    SketchGeom G;
    int C, nt;             /* k-mers per lane, lanes per strip (of the workgroup-per-strip passes: sketch_wave_kernel's lane holds nt / 4 k-mers) */
    uint64_t strips;       /* upper bound from the host-side lengths (exact for sequences without non-ACGT bytes): grids are sized without waiting for the device */
    WindowPass pass;
    bool big, direct;      /* BLOCK_MINIMA and the list pass behind WAVE: the kernel's BIG form; THRESH: the variant without staged keys */
    WaveShape shape;       /* WAVE */
    unsigned beside;       /* WAVE, two streams: wavefront slots per CU the resident workgroups take beside the other stream's kernels */
    int wgs_per_cu;        /* WAVE: NTL_SKW_WGS_PER_CU (tuning); 0: from `beside` */
    uint32_t chunk_budget; /* WAVE: NTL_SKW_BUDGET (0: resident wavefronts; tuning, tools/share_sweep.py) */
    uint32_t thresh;       /* keys below it are candidates; 0: no threshold */
    int dbg, force_redo;
    double expected_per_strip; /* candidates 4096 k-mers are expected to hold */
    bool dense_windows;    /* for the emit grid */
    bool lists;            /* the passes write per-strip lists of minimizers, not the bitmask */
    uint32_t slot, pool;   /* entries of a strip's list slot / of the pool behind the slots */
    bool fast() const { return pass >= WP_BLOCK_MINIMA; }
};

/* the shapes sketch_wave_kernel is instantiated for, once: the launch (with_wave_kernel) and the diagnostics (wave_shape_numbers,
   ntl_sketch_plan) read the same four template numbers */
#define NTL_WAVE_SHAPES(X) \
    X(WS_8_11_4, 8, 11, 4, 64) X(WS_8_15_6, 8, 15, 6, 64) X(WS_8_19_8, 8, 19, 8, 64) X(WS_4_19_8, 4, 19, 8, 64) \
    X(WS_8_19_7_L128, 8, 19, 7, 128) X(WS_4_11_4, 4, 11, 4, 64) X(WS_16_11_4, 16, 11, 4, 64)

template <typename F>
static void with_wave_kernel(WaveShape shape, F &&f)
{
    switch (shape) {
#define NTL_WAVE_CASE(id, waves, slots, rounds, cl) case id: return f(sketch_wave_kernel<waves, slots, rounds, cl>, 64u * waves);
    NTL_WAVE_SHAPES(NTL_WAVE_CASE)
#undef NTL_WAVE_CASE
    }
}

/* {wavefronts per workgroup, staging slots per lane, scan rounds, k-mers per lane} of a shape */
static void wave_shape_numbers(WaveShape shape, int32_t out[4])
{
    switch (shape) {
#define NTL_WAVE_CASE(id, waves, slots, rounds, cl) case id: out[0] = waves; out[1] = slots; out[2] = rounds; out[3] = cl; return;
    NTL_WAVE_SHAPES(NTL_WAVE_CASE)
#undef NTL_WAVE_CASE
    }
}
