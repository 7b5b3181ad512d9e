/*
 * Probe of the instruction wrappers (dev_intrin.h), block_excl_scan (dev_common.h) and the scan kernels (scan_kernels.h).
 * TEST TOOL ONLY.  One source, two builds (tests/probe/probelib.py): hipcc for gfx950 with -I ntlink_amd/csrc, and g++ with
 * tests/sim/include first, so that the same probe kernels run over the product's dev_intrin.h and over the SIMT mock's.
 *
 * Every lane reads its operands from an input table and writes its results to an output table: operand j of thread t is word
 * in[j * NT + t], result j is out[j * NT + t] (NT = threads of the one workgroup), unless said otherwise at the operation.  The
 * output table comes from the caller and goes back to it whole: what no lane writes keeps the caller's pattern.
 * The entry points allocate, copy, launch on the default stream, copy back and free; they return the HIP error code (0 = fine)
 * or -1 for tables too small for the operation (checked in front of every launch: no kernel here reads or writes beyond them).
 */
#include <utility>
#include "dev_common.h"
#include "dev_intrin.h"
#include "scan_kernels.h"

enum {
    OP_ALIGNBIT = 0, OP_BFE, OP_BFI, OP_SHL1_NE, OP_SHL1_LE, OP_SHL1_EQ, OP_SHL1_LT_DIFF, OP_LE4, OP_ROW_MIN16, OP_ROW_MAX16,
    OP_QUAD_MIN, OP_QUAD_SUM, OP_WAVE_MIN, OP_WAVE_INCL_SCAN, OP_MBCNT, OP_BREV, OP_DOUBLE, OP_SUB_SAT, OP_MIN3, OP_MUL_ADD_RN,
    OP_LOAD_U64_A1, OP_LOAD_U32_A1, OP_STORE_U64_A1, OP_LOAD4_A4, OP_STREAM, OP_LDS_LOAD2, OP_PUSH_TAGGED, OP_WAVE_SYNC,
    OP_READFIRSTLANE, OP_COUNT
};

#define PROBE_NT 256       /* the most threads of a probe workgroup (the LDS tables below are sized by it) */
#define PROBE_PUSH_T 128   /* ntl_lds_push_tagged<T> for T = 0 .. 127 */
#define PROBE_PUSH_WORDS 6 /* per lane and T: five LDS words (three pushed, two behind them) and the bytes the pointer moved */

/* words of input and output per thread */
static const struct { unsigned in, out; } op_words[OP_COUNT] = {
    /* ALIGNBIT */ {3, 1}, /* BFE */ {3, 1}, /* BFI */ {2, 1}, /* SHL1_NE */ {3, 1}, /* SHL1_LE */ {3, 1}, /* SHL1_EQ */ {3, 1},
    /* SHL1_LT_DIFF */ {3, 2}, /* LE4 */ {5, 1}, /* ROW_MIN16 */ {1, 1}, /* ROW_MAX16 */ {1, 1}, /* QUAD_MIN */ {1, 1},
    /* QUAD_SUM */ {1, 1}, /* WAVE_MIN */ {1, 1}, /* WAVE_INCL_SCAN */ {1, 1}, /* MBCNT */ {2, 1}, /* BREV */ {1, 1},
    /* DOUBLE */ {1, 1}, /* SUB_SAT */ {2, 1}, /* MIN3 */ {3, 1}, /* MUL_ADD_RN */ {6, 2}, /* LOAD_U64_A1 */ {4, 2},
    /* LOAD_U32_A1 */ {2, 1}, /* STORE_U64_A1 */ {2, 6}, /* LOAD4_A4 */ {8, 4}, /* STREAM */ {2, 2}, /* LDS_LOAD2 */ {2, 2},
    /* PUSH_TAGGED */ {4, PROBE_PUSH_T * PROBE_PUSH_WORDS}, /* WAVE_SYNC */ {2, 2}, /* READFIRSTLANE */ {1, 1}};

template <int T>
__device__ __forceinline__ void probe_push(uint32_t *slot, uint32_t mask, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t *out, int t, int nt)
{
    for (int j = 0; j < 5; j++) slot[j] = 0xC0FFEE00u + (uint32_t)j;
    uint32_t *p = slot;
    ntl_lds_push_tagged<T>(p, mask, v0);
    ntl_lds_push_tagged<T>(p, mask, v1);
    ntl_lds_push_tagged<T>(p, mask, v2);
    uint32_t *o = out + ((size_t)T * nt + t) * PROBE_PUSH_WORDS;
    for (int j = 0; j < 5; j++) o[j] = slot[j];
    o[5] = (uint32_t)((const char *)p - (const char *)slot);
}

template <int... T>
__device__ __forceinline__ void probe_push_all(std::integer_sequence<int, T...>, uint32_t *slot, uint32_t mask, uint32_t v0, uint32_t v1,
                                               uint32_t v2, uint32_t *out, int t, int nt)
{
    (probe_push<T>(slot, mask, v0, v1, v2, out, t, nt), ...);
}

/* the MASKs of ntl_bfi<MASK>: 1 and 2 are the product's (srol1, sror1), 0 and all ones the ends */
__device__ __forceinline__ uint32_t probe_bfi(int which, uint32_t a, uint32_t b)
{
    switch (which) { /* uniform */
    case 0: return ntl_bfi<0u>(a, b);
    case 1: return ntl_bfi<1u>(a, b);
    case 2: return ntl_bfi<2u>(a, b);
    default: return ntl_bfi<0xFFFFFFFFu>(a, b);
    }
}

/* one workgroup of nt <= PROBE_NT threads; `active` = the lanes (of every wavefront) that run OP_MBCNT, the only operation that is
   probed inside divergent code */
__global__ __launch_bounds__(PROBE_NT) void probe_kernel(int op, int param, const uint32_t *in, uint32_t *out, unsigned long long active)
{
    __shared__ uint2 s_tab[PROBE_NT];
    __shared__ uint32_t s_slot[PROBE_NT * 5];
    __shared__ uint32_t s_x[PROBE_NT];
    const int t = threadIdx.x, nt = blockDim.x, l = t & 63;
#define IN(j) in[(j) * nt + t]
#define OUT(j) out[(j) * nt + t]
    switch (op) { /* uniform */
    case OP_ALIGNBIT: OUT(0) = ntl_alignbit(IN(0), IN(1), IN(2)); break;
    case OP_BFE: OUT(0) = ntl_bfe(IN(0), IN(1), IN(2)); break;
    case OP_BFI: OUT(0) = probe_bfi(param, IN(0), IN(1)); break;
    case OP_SHL1_NE: OUT(0) = ntl_shl1_or_ne(IN(0), IN(1), IN(2)); break;
    case OP_SHL1_LE: OUT(0) = ntl_shl1_or_le(IN(0), IN(1), IN(2)); break;
    case OP_SHL1_EQ: OUT(0) = ntl_shl1_or_eq(IN(0), IN(1), IN(2)); break;
    case OP_SHL1_LT_DIFF: {
        uint32_t d;
        OUT(0) = ntl_shl1_or_lt_diff(IN(0), IN(1), IN(2), d);
        OUT(1) = d;
        break;
    }
    case OP_LE4: OUT(0) = ntl_le4_mask(IN(0), IN(1), IN(2), IN(3), IN(4)); break;
    case OP_ROW_MIN16: OUT(0) = ntl_row_min16(IN(0)); break;
    case OP_ROW_MAX16: OUT(0) = ntl_row_max16(IN(0)); break;
    case OP_QUAD_MIN: OUT(0) = ntl_quad_min(IN(0)); break;
    case OP_QUAD_SUM: OUT(0) = ntl_quad_sum(IN(0)); break;
    case OP_WAVE_MIN: OUT(0) = ntl_wave_min(IN(0)); break;
    case OP_WAVE_INCL_SCAN: OUT(0) = ntl_wave_incl_scan(IN(0)); break;
    case OP_MBCNT:
        if ((active >> l) & 1ull) OUT(0) = ntl_mbcnt(((unsigned long long)IN(1) << 32) | IN(0));
        break;
    case OP_BREV: OUT(0) = ntl_brev(IN(0)); break;
    case OP_DOUBLE: OUT(0) = ntl_double(IN(0)); break;
    case OP_SUB_SAT: OUT(0) = ntl_sub_sat(IN(0), IN(1)); break;
    case OP_MIN3: OUT(0) = ntl_min3(IN(0), IN(1), IN(2)); break;
    case OP_MUL_ADD_RN: { /* three tables of nt doubles -> one */
        const double *d = (const double *)in;
        ((double *)out)[t] = ntl_mul_add_rn(d[t], d[nt + t], d[2 * nt + t]);
        break;
    }
    case OP_LOAD_U64_A1: { /* 16 bytes per thread, read at byte t & 7 of them */
        const uint64_t v = ntl_load_u64_a1((const uint8_t *)in + 16 * t + (t & 7));
        OUT(0) = (uint32_t)v; OUT(1) = (uint32_t)(v >> 32);
        break;
    }
    case OP_LOAD_U32_A1: OUT(0) = ntl_load_u32_a1((const uint8_t *)in + 8 * t + (t & 3)); break; /* 8 bytes per thread */
    case OP_STORE_U64_A1: /* 24 bytes of output per thread, written at bytes 4 + (t & 7) .. 11 + (t & 7) of them */
        ntl_store_u64_a1((uint8_t *)out + 24 * t + 4 + (t & 7), ((uint64_t)IN(1) << 32) | IN(0));
        break;
    case OP_LOAD4_A4: { /* 8 words per thread (32 bytes: a 16-byte-aligned base), read from word t & 3 of them */
        const uint4 v = ntl_load4_a4(in + 8 * t + (t & 3));
        OUT(0) = v.x; OUT(1) = v.y; OUT(2) = v.z; OUT(3) = v.w;
        break;
    }
    case OP_STREAM: ntl_stream_store((uint64_t *)out + t, ntl_stream_load((const uint64_t *)in + t)); break;
    case OP_LDS_LOAD2: { /* the table staged in LDS, read back from another thread's slot */
        s_tab[t] = make_uint2(IN(0), IN(1));
        __syncthreads();
        const uint2 v = ntl_lds_load2_ordered(&s_tab[(t * 7 + 3) % nt]);
        OUT(0) = v.x; OUT(1) = v.y;
        break;
    }
    case OP_PUSH_TAGGED: /* out: PROBE_PUSH_WORDS words per (T, thread) */
        probe_push_all(std::make_integer_sequence<int, PROBE_PUSH_T>(), s_slot + 5 * t, IN(0), IN(1), IN(2), IN(3), out, t, nt);
        break;
    case OP_WAVE_SYNC: { /* lanes of a wavefront exchange through LDS with no workgroup barrier */
        uint32_t *x = s_x + (t & ~63);
        x[l] = IN(0);
        ntl_wave_sync();
        OUT(0) = x[(l + 1) & 63];
        ntl_wave_sync();
        x[l] = IN(1);
        ntl_wave_sync();
        OUT(1) = x[(l + 63) & 63];
        break;
    }
    case OP_READFIRSTLANE: OUT(0) = ntl_readfirstlane(IN(0)); break;
    default: break;
    }
#undef IN
#undef OUT
}

/* block_excl_scan<NT> twice in a row over the same s_tmp: in = two tables, out = prefix 1, total 1, prefix 2, total 2 */
template <int NT>
__global__ __launch_bounds__(NT) void probe_block_scan_kernel(const uint32_t *in, uint32_t *out)
{
    __shared__ uint32_t s_tmp[NT];
    const int t = threadIdx.x;
    uint32_t total1, total2;
    const uint32_t r1 = block_excl_scan<NT>(in[t], s_tmp, total1);
    const uint32_t r2 = block_excl_scan<NT>(in[NT + t], s_tmp, total2);
    out[t] = r1; out[NT + t] = total1; out[2 * NT + t] = r2; out[3 * NT + t] = total2;
}

/* ---------------------------------------------------------------- host side */

#define PCHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

namespace {
/* device memory of one call; release() is the checked way out, the destructor the one behind an error */
struct Buf {
    void *p = nullptr;
    ~Buf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
    hipError_t up(const void *h, size_t bytes) { return bytes ? hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) : hipSuccess; }
    hipError_t down(void *h, size_t bytes) { return bytes ? hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    hipError_t release() { void *q = p; p = nullptr; return q ? hipFree(q) : hipSuccess; }
    uint32_t *u32() { return (uint32_t *)p; }
};
const hipStream_t DEFAULT_STREAM = (hipStream_t)0;
}  // namespace

extern "C" int probe_op_count(void) { return OP_COUNT; }
extern "C" int probe_push_t(void) { return PROBE_PUSH_T; }

/* one workgroup of nthreads (whole wavefronts, <= 256) runs operation op; in_words / out_words: what the caller's tables hold */
extern "C" int probe_run(int op, int param, const uint32_t *in, uint64_t in_words, uint32_t *out, uint64_t out_words, uint32_t nthreads,
                         unsigned long long active)
{
    if (op < 0 || op >= OP_COUNT || nthreads == 0 || nthreads % 64 || nthreads > PROBE_NT) return -1;
    if (in_words < (uint64_t)op_words[op].in * nthreads || out_words < (uint64_t)op_words[op].out * nthreads) return -1;
    Buf din, dout;
    PCHK(din.alloc(in_words * 4)); PCHK(dout.alloc(out_words * 4));
    PCHK(din.up(in, in_words * 4)); PCHK(dout.up(out, out_words * 4));
    hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(nthreads), 0, DEFAULT_STREAM, op, param, (const uint32_t *)din.u32(), dout.u32(), active);
    PCHK(hipGetLastError());
    PCHK(hipDeviceSynchronize());
    PCHK(dout.down(out, out_words * 4));
    PCHK(din.release()); PCHK(dout.release());
    return 0;
}

/* in: 2 * nt words, out: 4 * nt words; nt = 128, 256 or 512 (what the product instantiates) */
extern "C" int probe_block_scan(uint32_t nt, const uint32_t *in, uint32_t *out)
{
    if (nt != 128 && nt != 256 && nt != 512) return -1;
    Buf din, dout;
    PCHK(din.alloc(2 * nt * 4)); PCHK(dout.alloc(4 * nt * 4));
    PCHK(din.up(in, 2 * nt * 4)); PCHK(dout.up(out, 4 * nt * 4));
    if (nt == 128) hipLaunchKernelGGL((probe_block_scan_kernel<128>), dim3(1), dim3(128), 0, DEFAULT_STREAM, (const uint32_t *)din.u32(), dout.u32());
    else if (nt == 256) hipLaunchKernelGGL((probe_block_scan_kernel<256>), dim3(1), dim3(256), 0, DEFAULT_STREAM, (const uint32_t *)din.u32(), dout.u32());
    else hipLaunchKernelGGL((probe_block_scan_kernel<512>), dim3(1), dim3(512), 0, DEFAULT_STREAM, (const uint32_t *)din.u32(), dout.u32());
    PCHK(hipGetLastError());
    PCHK(hipDeviceSynchronize());
    PCHK(dout.down(out, 4 * nt * 4));
    PCHK(din.release()); PCHK(dout.release());
    return 0;
}

extern "C" uint64_t probe_scan_tile_count(uint64_t n) { return scan_tile_count(n); }
extern "C" uint64_t probe_scan_self_max_tiles(void) { return SCAN_SELF_MAX_TILES; }
extern "C" uint32_t probe_scan_tile(void) { return SCAN_TILE; }

/* scan_launch, the launch sequence of the product's device_scan.
 *   out      batch * (n + 1) + out_guard words, sent up and brought back whole; with inplace != 0 it holds the input
 *   in       batch * (n + 1) words (inplace == 0), sent up and brought back into in_back
 *   tile     tile_words >= scan_tile_count(n) * batch words, sent up and brought back whole
 *   sums     null, or sums_words >= batch words, sent up and brought back whole */
extern "C" int probe_scan(const uint32_t *in, uint32_t *in_back, uint32_t *out, uint64_t out_guard, uint64_t n, uint32_t batch, int inplace,
                          uint32_t *sums, uint64_t sums_words, uint64_t self_max_tiles, uint32_t *tile, uint64_t tile_words)
{
    if (batch == 0 || tile_words < scan_tile_count(n) * batch || (sums && sums_words < batch) || (!inplace && (!in || !in_back))) return -1;
    const uint64_t words = (uint64_t)batch * (n + 1);
    Buf din, dout, dtile, dsums;
    PCHK(dout.alloc((words + out_guard) * 4)); PCHK(dout.up(out, (words + out_guard) * 4));
    PCHK(dtile.alloc(tile_words * 4)); PCHK(dtile.up(tile, tile_words * 4));
    if (!inplace) { PCHK(din.alloc(words * 4)); PCHK(din.up(in, words * 4)); }
    if (sums) { PCHK(dsums.alloc(sums_words * 4)); PCHK(dsums.up(sums, sums_words * 4)); }
    scan_launch(DEFAULT_STREAM, inplace ? (const uint32_t *)dout.u32() : (const uint32_t *)din.u32(), dout.u32(), n, batch, dtile.u32(),
                sums ? dsums.u32() : nullptr, self_max_tiles);
    PCHK(hipGetLastError());
    PCHK(hipDeviceSynchronize());
    PCHK(dout.down(out, (words + out_guard) * 4));
    PCHK(dtile.down(tile, tile_words * 4));
    if (!inplace) PCHK(din.down(in_back, words * 4));
    if (sums) PCHK(dsums.down(sums, sums_words * 4));
    PCHK(din.release()); PCHK(dout.release()); PCHK(dtile.release()); PCHK(dsums.release());
    return 0;
}

/* scan_tiles_kernel alone, in place, as the emit stage launches it: gy arrays of n words side by side in `data`
 *   data     data_words >= gy * n words, sent up and brought back whole
 *   total    total_words >= (gy - 1) * total_stride + 1 words, sent up and brought back whole
 *   extra    null, or extra_words >= gy words, sent up and brought back whole */
extern "C" int probe_scan_tiles(uint32_t *data, uint64_t data_words, uint64_t n, uint32_t gy, uint32_t *total, uint64_t total_stride,
                                uint64_t total_words, uint32_t *extra, uint64_t extra_words)
{
    if (gy == 0 || data_words < (uint64_t)gy * n || total_words < (uint64_t)(gy - 1) * total_stride + 1 || (extra && extra_words < gy)) return -1;
    Buf ddata, dtotal, dextra;
    PCHK(ddata.alloc(data_words * 4)); PCHK(ddata.up(data, data_words * 4));
    PCHK(dtotal.alloc(total_words * 4)); PCHK(dtotal.up(total, total_words * 4));
    if (extra) { PCHK(dextra.alloc(extra_words * 4)); PCHK(dextra.up(extra, extra_words * 4)); }
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(1, gy), dim3(SCAN_NT), 0, DEFAULT_STREAM, ddata.u32(), n, dtotal.u32(), total_stride,
                       extra ? dextra.u32() : (uint32_t *)nullptr);
    PCHK(hipGetLastError());
    PCHK(hipDeviceSynchronize());
    PCHK(ddata.down(data, data_words * 4));
    PCHK(dtotal.down(total, total_words * 4));
    if (extra) PCHK(dextra.down(extra, extra_words * 4));
    PCHK(ddata.release()); PCHK(dtotal.release()); PCHK(dextra.release());
    return 0;
}
