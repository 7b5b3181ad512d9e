"""Operand tables and definitions for the probe of the instruction wrappers (tests/probe): for every wrapper of dev_intrin.h a table
of operands and the comment above the wrapper restated in NumPy -- uint64 arithmetic masked to 32 bits, written from the comment, not
from either body.  check_*(probe) runs a table through the probe (tests/probe/probelib.py: the product's bodies on the GPU, the
mock's on the CPU) and compares exactly; tests/test_intrinsics.py calls every check both ways."""
import functools
from fractions import Fraction

import numpy as np

from probe.probelib import ALL_LANES, FILL

M32 = np.uint64(0xFFFFFFFF)
NT = 256
EDGES = (0, 1, 2, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF)
BFI_MASKS = (0, 1, 2, 0xFFFFFFFF)  # probe_bfi's table: 1 and 2 are the product's (dev_common.h srol1, sror1)
BLOCK_SCAN_NT = (128, 256, 512)    # block_excl_scan<NT>: sketch_fast_kernel<128>, SCAN_NT / EMIT_NT / SK_NT = 256, SK_NT_LONG = 512
PUSH_CANARY = 0xC0FFEE00           # probe_push: slot word j holds PUSH_CANARY + j before the pushes

# wrapper (or macro) of dev_intrin.h -> the check that probes it
PROBED = {
    "ntl_alignbit": "alignbit", "ntl_bfe": "bfe", "ntl_bfi": "bfi", "ntl_shl1_or_ne": "shl1", "ntl_shl1_or_le": "shl1",
    "ntl_shl1_or_eq": "shl1", "ntl_shl1_or_lt_diff": "shl1", "ntl_le4_mask": "le4_mask", "ntl_row_min16": "cross_lane",
    "ntl_row_max16": "cross_lane", "ntl_quad_min": "cross_lane", "ntl_quad_sum": "cross_lane", "ntl_wave_min": "cross_lane",
    "ntl_wave_incl_scan": "cross_lane", "ntl_mbcnt": "mbcnt", "ntl_brev": "unary", "ntl_double": "unary", "ntl_sub_sat": "sub_sat_min3",
    "ntl_min3": "sub_sat_min3", "ntl_mul_add_rn": "mul_add_rn", "ntl_load_u64_a1": "memory", "ntl_load_u32_a1": "memory",
    "ntl_store_u64_a1": "memory", "ntl_load4_a4": "memory", "ntl_stream_load": "memory", "ntl_stream_store": "memory",
    "ntl_lds_load2_ordered": "memory", "ntl_lds_push_tagged": "lds_push_tagged", "ntl_wave_sync": "wave_sync",
    "ntl_readfirstlane": "readfirstlane",
}
# names with no value to compare
EXEMPT = {
    "NTL_MAIN_STREAM_SGPRS": "a register-budget attribute of kernels",
    "NTL_PRIO_LATENCY_BOUND": "an issue-priority hint, no result",
    "NTL_OPAQUE": "hides a value from the optimiser, the value is unchanged",
    "NTL_LDS_CU64": "a pointer cast (address space), no arithmetic",
    "ntl_lds_cu64": "the type NTL_LDS_CU64 casts to",
}


def u32(x):
    return np.asarray(x, np.uint64).astype(np.uint32)


def rng(seed):
    return np.random.default_rng(seed)


def rand32(r, n):
    return r.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def product(*cols):
    """every combination of the columns' values, one array per column"""
    grid = np.meshgrid(*[np.asarray(c, np.uint64) for c in cols], indexing="ij")
    return [g.ravel().astype(np.uint32) for g in grid]


def run_rows(probe, op, cols, n_out, param=0):
    """an elementwise operation over tables of any length: workgroups of NT rows, the last one padded with its first row"""
    n = len(cols[0])
    outs = [np.empty(n, np.uint32) for _ in range(n_out)]
    for lo in range(0, n, NT):
        part = [np.resize(c[lo:lo + NT], NT) if len(c[lo:lo + NT]) < NT else c[lo:lo + NT] for c in cols]
        got = probe.run(op, np.stack(part), n_out * NT, param=param).reshape(n_out, NT)
        m = min(NT, n - lo)
        for j in range(n_out):
            outs[j][lo:lo + m] = got[j, :m]
    return outs


def same(got, want, what, *operands):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        ops = ", ".join(hex(int(o[i])) for o in operands)
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at row {i} ({ops}): got {int(got[i]):#x}, the definition gives {int(want[i]):#x}")


# ---------------------------------------------------------------- elementwise integer wrappers

def check_alignbit(probe):
    """({hi,lo} >> sh)[31:0], sh in 0..31"""
    vals = (0, 1, 0x80000000, 0xFFFFFFFF) + tuple(int(v) for v in rand32(rng(1), 3))
    hi, lo, sh = product(vals, vals, (0, 1, 15, 16, 31))
    want = (((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)) >> sh.astype(np.uint64)) & M32
    same(run_rows(probe, "alignbit", [hi, lo, sh], 1)[0], u32(want), "ntl_alignbit", hi, lo, sh)


def check_bfe(probe):
    """(x >> off) & ((1 << width) - 1) over the whole contract, off and width in 0..31 each (the call sites: width 8, off 0/8/16/24)"""
    x, off, width = product((0xFFFFFFFF, 0x80000001, 0x12345678) + tuple(int(v) for v in rand32(rng(2), 2)), range(32), range(32))
    want = (x.astype(np.uint64) >> off.astype(np.uint64)) & ((np.uint64(1) << width.astype(np.uint64)) - np.uint64(1))
    assert ((off == 24) & (width == 8)).any() and ((off == 31) & (width == 31)).any()
    same(run_rows(probe, "bfe", [x, off, width], 1)[0], u32(want), "ntl_bfe", x, off, width)


def check_bfi(probe):
    """(a & mask) | (b & ~mask) for every MASK the product instantiates, 0 and all ones"""
    vals = EDGES + tuple(int(v) for v in rand32(rng(3), 4))
    a, b = product(vals, vals)
    for which, mask in enumerate(BFI_MASKS):
        m = np.uint64(mask)
        want = (a.astype(np.uint64) & m) | (b.astype(np.uint64) & (~m & M32))
        same(run_rows(probe, "bfi", [a, b], 1, param=which)[0], u32(want), f"ntl_bfi<{mask:#x}>", a, b)


def compare_pairs():
    """(a, b): equal, one apart either way, the ends of the range against each other, random"""
    r = rng(4)
    base = np.array(list(EDGES) + [int(v) for v in rand32(r, 8)], np.uint64)
    a = np.concatenate([base, base, base, [0, 0xFFFFFFFF], rand32(r, 16)]).astype(np.uint64)
    b = np.concatenate([base, (base + np.uint64(1)) & M32, (base - np.uint64(1)) & M32, [0xFFFFFFFF, 0], rand32(r, 16)]).astype(np.uint64)
    return a, b


def check_shl1(probe):
    """(acc << 1) | (a != b), (a <= b), (a == b), (a < b) with d = a - b wrapping: the bit shifted out of acc vanishes"""
    a, b = compare_pairs()
    accs = np.array([0, 1, 0x80000000, 0xFFFFFFFF, 0x40000001, 0xC0000000, 0x2AAAAAAA], np.uint64)
    acc = np.repeat(accs, len(a))
    a, b = np.tile(a, len(accs)), np.tile(b, len(accs))
    assert ((acc >> np.uint64(31)) == 1).any() and (a == b).any() and (a < b).any() and (a > b).any()
    cols = [u32(acc), u32(a), u32(b)]
    sh = (acc << np.uint64(1)) & M32
    for op, bit in (("shl1_or_ne", a != b), ("shl1_or_le", a <= b), ("shl1_or_eq", a == b)):
        same(run_rows(probe, op, cols, 1)[0], u32(sh | bit.astype(np.uint64)), "ntl_" + op, *cols)
    r, d = run_rows(probe, "shl1_or_lt_diff", cols, 2)
    same(r, u32(sh | (a < b).astype(np.uint64)), "ntl_shl1_or_lt_diff", *cols)
    want_d = (a - b) & M32  # uint64 arithmetic wraps at 2^64, a multiple of 2^32
    assert (want_d[a < b] > 0x7FFFFFFF).any()  # wrapped differences are in the table
    same(d, u32(want_d), "ntl_shl1_or_lt_diff's d", *cols)


def check_le4_mask(probe):
    """bit i: k_i <= lim, bit 4 set.  Every one of the sixteen patterns at every lim where both outcomes exist, with k_i at the limit,
    one above it and at the far ends: a swapped operand order gives another pattern"""
    rows = []
    for lim in (0, 1, 1000, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF):
        for pat in range(16):
            for le, gt in ((lim, lim + 1), (0, 0xFFFFFFFF), (lim // 2, lim + (0xFFFFFFFF - lim + 1) // 2)):
                ks = [(le if (pat >> i) & 1 else gt) for i in range(4)]
                if all(k <= 0xFFFFFFFF for k in ks) and (gt > lim or pat == 15):
                    rows.append(ks + [lim])
    r = rng(5)
    rows += [[int(v) for v in rand32(r, 5)] for _ in range(64)]
    t = np.array(rows, np.uint64)
    k, lim = [t[:, i] for i in range(4)], t[:, 4]
    want = np.uint64(16) | sum(((k[i] <= lim).astype(np.uint64) << np.uint64(i)) for i in range(4))
    for lm in (0, 0xFFFFFFFF):
        assert (lim == lm).any()
    assert {int(w) for w in want[lim == 1000]} == set(range(16, 32))  # all sixteen outcomes
    cols = [u32(c) for c in (*k, lim)]
    same(run_rows(probe, "le4_mask", cols, 1)[0], u32(want), "ntl_le4_mask", *cols)


def check_unary(probe):
    """bit reversal; x + x"""
    x = np.concatenate([np.array(EDGES, np.uint64), np.uint64(1) << np.arange(32, dtype=np.uint64), rand32(rng(6), 64)]).astype(np.uint64)
    rev = np.zeros_like(x)
    for i in range(32):
        rev |= ((x >> np.uint64(i)) & np.uint64(1)) << np.uint64(31 - i)
    same(run_rows(probe, "brev", [u32(x)], 1)[0], u32(rev), "ntl_brev", x)
    same(run_rows(probe, "double", [u32(x)], 1)[0], u32((x + x) & M32), "ntl_double", x)


def check_sub_sat_min3(probe):
    """a - b, 0 where it would wrap; the minimum of three"""
    a, b = compare_pairs()
    assert (a < b).any() and (a == b).any() and (a == b + np.uint64(1)).any()
    same(run_rows(probe, "sub_sat", [u32(a), u32(b)], 1)[0], u32(np.where(a >= b, a - b, np.uint64(0)) & M32), "ntl_sub_sat", a, b)
    vals = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF) + tuple(int(v) for v in rand32(rng(7), 3))
    x, y, z = product(vals, vals, vals)
    same(run_rows(probe, "min3", [x, y, z], 1)[0], np.minimum(np.minimum(x, y), z), "ntl_min3", x, y, z)


# ---------------------------------------------------------------- cross-lane wrappers (all 64 lanes active)

@functools.lru_cache(maxsize=None)
def lane_vectors():
    """u32[V][64], V a multiple of 4: the least value (0) in every lane position in turn with the greatest (0xFFFFFFFF) seven lanes
    on, a single 1 in every lane in turn, ties, all-equal inputs, sums that wrap 2^32"""
    r = rng(8)
    vs = []
    for j in range(64):
        v = r.integers(1000, 1 << 31, 64, dtype=np.uint64)
        v[j] = 0
        v[(j + 7) & 63] = 0xFFFFFFFF
        vs.append(v)
    for j in range(64):
        v = np.zeros(64, np.uint64)
        v[j] = 1
        vs.append(v)
    vs += [r.integers(0, 3, 64, dtype=np.uint64) for _ in range(3)]                      # ties everywhere
    vs += [r.integers(0, 3, 64, dtype=np.uint64) + np.uint64(0xFFFFFFFD) for _ in range(2)]  # ties at the top, sums that wrap
    vs += [np.full(64, c, np.uint64) for c in (0, 7, 0x80000000, 0xFFFFFFFF)]           # all equal
    vs += [r.integers(0, 1 << 32, 64, dtype=np.uint64) for _ in range(3)]                # random: every partial sum wraps
    assert len(vs) % 4 == 0
    return np.array(vs, np.uint64)


def cross_lane_definitions(v):
    """v: u64[V][64] -> {op: u64[V][64]}"""
    def groups(width, f):
        return np.repeat(f(v.reshape(len(v), 64 // width, width), axis=2), width, axis=1)
    return {"row_min16": groups(16, np.min), "row_max16": groups(16, np.max), "quad_min": groups(4, np.min),
            "quad_sum": groups(4, np.sum) & M32, "wave_min": groups(64, np.min), "wave_incl_scan": np.cumsum(v, axis=1) & M32}


def check_cross_lane(probe):
    """minimum / maximum / sum over quads, rows of 16 and the wavefront, the inclusive scan: four wavefronts with a vector each"""
    v = lane_vectors()
    want = cross_lane_definitions(v)
    assert (v.sum(axis=1) > 0xFFFFFFFF).any()
    for op, w in want.items():
        for lo in range(0, len(v), 4):
            got = probe.run(op, u32(v[lo:lo + 4]), NT).reshape(4, 64)
            for q in range(4):
                bad = np.flatnonzero(got[q] != u32(w[lo + q]))
                assert bad.size == 0, (f"ntl_{op}, vector {lo + q} = {[hex(int(x)) for x in v[lo + q]]}: lanes {bad.tolist()} hold "
                                       f"{[hex(int(x)) for x in got[q][bad]]}, the definition gives {[hex(int(x)) for x in w[lo + q][bad]]}")


MBCNT_MASKS = (0, (1 << 64) - 1, 1, 1 << 31, 1 << 32, 1 << 63, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA)
ACTIVE_SETS = (ALL_LANES, 0xAAAAAAAAAAAAAAAA, ALL_LANES & ~((1 << 37) - 1), 1 << 41)  # all, odd lanes, lanes >= 37, lane 41 alone


def check_mbcnt(probe):
    """set bits of `mask` below this lane, for any set of active lanes; an inactive lane's output is untouched"""
    r = rng(9)
    masks = list(MBCNT_MASKS) + [int(x) for x in r.integers(0, 1 << 63, 4, dtype=np.uint64) * 2 + r.integers(0, 2, 4, dtype=np.uint64)]
    lanes = np.arange(NT) & 63
    for active in ACTIVE_SETS:
        on = np.array([(active >> int(l)) & 1 for l in lanes], bool)
        for lo in range(0, len(masks), 4):  # a mask per wavefront
            m = np.repeat(np.array(masks[lo:lo + 4], np.uint64), 64)
            want = np.array([bin(int(mm) & ((1 << int(l)) - 1)).count("1") for mm, l in zip(m, lanes)], np.uint32)
            got = probe.run("mbcnt", np.stack([u32(m & M32), u32(m >> np.uint64(32))]), NT, active=active)
            same(got[on], want[on], f"ntl_mbcnt, active lanes {active:#x}", m[on], lanes[on])
            assert (got[~on] == FILL).all(), f"ntl_mbcnt, active lanes {active:#x}: an inactive lane wrote its output"


def check_readfirstlane(probe):
    """the value of the first active lane in every lane; every call site is wave-uniform, so that is lane 0"""
    v = rand32(rng(10), NT)
    same(probe.run("readfirstlane", v, NT), np.repeat(v[::64], 64), "ntl_readfirstlane", v)


def check_wave_sync(probe):
    """lane l writes slot l, reads slot l + 1; writes again, reads slot l - 1 (mod 64), within its own wavefront"""
    a, b = rand32(rng(11), NT).reshape(4, 64), rand32(rng(12), NT).reshape(4, 64)
    got = probe.run("wave_sync", np.stack([a.ravel(), b.ravel()]), 2 * NT).reshape(2, 4, 64)
    same(got[0].ravel(), np.roll(a, -1, axis=1).ravel(), "ntl_wave_sync, first hand-off", a.ravel())
    same(got[1].ravel(), np.roll(b, 1, axis=1).ravel(), "ntl_wave_sync, second hand-off", b.ravel())


# ---------------------------------------------------------------- x * d + k with two roundings

def to_float(q):
    """a Fraction rounded once to the nearest double (int / int is correctly rounded)"""
    return q.numerator / q.denominator


@functools.lru_cache(maxsize=None)
def mul_add_cases():
    """(x, d, k) float64 tables: at least 20 triples whose fused result differs from the two-rounding one, found with exact
    arithmetic, and values of the size the call site sees (bin/ntlink_utils.py:230-231: small x, distances up to 2^32, small k)"""
    r = rng(13)
    cand = list(zip(r.random(4000).tolist(), r.integers(1, 1 << 32, 4000).astype(float).tolist(), (r.random(4000) * 100).tolist()))
    differ = []
    for x, d, k in cand:
        p = Fraction(x) * Fraction(d)
        fused, two = to_float(p + Fraction(k)), to_float(Fraction(to_float(p)) + Fraction(k))
        assert two == x * d + k  # Python floats round twice
        if fused != two:
            differ.append((x, d, k))
    assert len(differ) >= 20, len(differ)
    usual = [(x, float(d), float(k)) for x in (0.0, 1.0, 0.05, 0.5, 1e-5) for d in (0, 1, 15, 1000, 123457, (1 << 31) + 1, (1 << 32) - 1, 1 << 32)
             for k in (0, 1, 13, 64)]
    rows = differ[:40] + usual + cand[:NT]
    rows = rows[:(len(rows) // NT) * NT] if len(rows) % NT else rows
    t = np.array(rows, np.float64)
    return t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy(), min(len(differ), 40)


def check_mul_add_rn(probe):
    """float64 bit patterns against NumPy's x * d, then + k"""
    x, d, k, _ = mul_add_cases()
    want = (x * d + k).view(np.uint64)
    for lo in range(0, len(x), NT):
        s = slice(lo, lo + NT)
        got = probe.run("mul_add_rn", np.stack([x[s], d[s], k[s]]), 2 * NT).view(np.uint64)
        same(got, want[s], "ntl_mul_add_rn", x[s].view(np.uint64), d[s].view(np.uint64), k[s].view(np.uint64))


# ---------------------------------------------------------------- memory wrappers

def check_memory(probe):
    """unaligned loads and the unaligned store at every byte offset, the four-word load at every word offset, the streaming pair,
    the ordered LDS read"""
    r = rng(14)
    t = np.arange(NT)
    raw = r.integers(0, 256, 16 * NT, dtype=np.uint8)
    want = np.array([int.from_bytes(raw[16 * i + (i & 7):16 * i + (i & 7) + 8].tobytes(), "little") for i in t], np.uint64)
    got = probe.run("load_u64_a1", raw, 2 * NT).reshape(2, NT).astype(np.uint64)
    same(got[0] | (got[1] << np.uint64(32)), want, "ntl_load_u64_a1 (thread t reads at byte offset t & 7)", t)

    raw = r.integers(0, 256, 8 * NT, dtype=np.uint8)
    want = np.array([int.from_bytes(raw[8 * i + (i & 3):8 * i + (i & 3) + 4].tobytes(), "little") for i in t], np.uint32)
    same(probe.run("load_u32_a1", raw, NT), want, "ntl_load_u32_a1 (thread t reads at byte offset t & 3)", t)

    v = r.integers(0, 1 << 63, NT, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    got = probe.run("store_u64_a1", np.stack([u32(v & M32), u32(v >> np.uint64(32))]), 6 * NT).view(np.uint8)
    want = np.full(6 * NT, FILL, np.uint32).view(np.uint8).copy()  # guard bytes on both sides of every store
    for i in t:
        want[24 * i + 4 + (i & 7):24 * i + 12 + (i & 7)] = np.frombuffer(int(v[i]).to_bytes(8, "little"), np.uint8)
    same(got, want, "ntl_store_u64_a1 (thread t writes at byte 4 + (t & 7) of its 24; the rest are guards)", np.arange(24 * NT) // 24)

    w = rand32(r, 8 * NT)
    got = probe.run("load4_a4", w, 4 * NT).reshape(4, NT)
    for j in range(4):
        same(got[j], w[8 * t + (t & 3) + j], f"ntl_load4_a4 word {j} (thread t reads from word offset t & 3)", t)

    w = rand32(r, 2 * NT)
    same(probe.run("stream", w, 2 * NT), w, "ntl_stream_load -> ntl_stream_store", np.arange(2 * NT))

    x, y = rand32(r, NT), rand32(r, NT)
    got = probe.run("lds_load2_ordered", np.stack([x, y]), 2 * NT).reshape(2, NT)
    src = (t * 7 + 3) % NT
    same(got[0], x[src], "ntl_lds_load2_ordered .x", t)
    same(got[1], y[src], "ntl_lds_load2_ordered .y", t)


def check_lds_push_tagged(probe):
    """*p++ = (v & ~mask) | (T & mask), three times in a row, for T = 0 .. 127 (the product's: 0 and the rolling steps 1 .. 127; both
    sides of the inline-constant limit 64): the stored words, the two words behind them, the pointer 12 bytes on"""
    r = rng(15)
    t = np.arange(NT)
    mask = np.array([0, 0xFF, 0xFFFFFFFF, 63, 127], np.uint64)[t % 5]  # 63 and 127 are the product's (TAGM)
    v = [rand32(r, NT).astype(np.uint64) for _ in range(3)]
    v[0][:8] = EDGES
    n_t = probe.push_t
    assert n_t == 128
    got = probe.run("lds_push_tagged", np.stack([u32(mask), *[u32(x) for x in v]]), n_t * NT * 6).reshape(n_t, NT, 6)
    for T in range(n_t):
        for j in range(3):
            want = (v[j] & (~mask & M32)) | (np.uint64(T) & mask)
            same(got[T, :, j], u32(want), f"ntl_lds_push_tagged<{T}>, push {j}", mask, v[j])
        for j in (3, 4):
            assert (got[T, :, j] == PUSH_CANARY + j).all(), f"ntl_lds_push_tagged<{T}>: the word {j - 2} behind the pushes changed"
        assert (got[T, :, 5] == 12).all(), f"ntl_lds_push_tagged<{T}>: the pointer moved by {set(got[T, :, 5].tolist())} bytes, not 12"


# ---------------------------------------------------------------- block_excl_scan

def check_block_excl_scan(probe):
    """exclusive prefix and total over a workgroup, twice in a row over the same LDS words, for every NT of the product"""
    r = rng(16)
    for nt in BLOCK_SCAN_NT:
        tables = [np.zeros(nt, np.uint64), np.ones(nt, np.uint64), r.integers(0, 1 << 20, nt, dtype=np.uint64),
                  np.full(nt, 0xFFFFFFFF, np.uint64), r.integers(0, 1 << 32, nt, dtype=np.uint64)]
        single = np.zeros(nt, np.uint64)
        single[nt - 1] = 5  # only the last thread counts: its own prefix stays 0
        tables.append(single)
        for a, b in zip(tables, tables[1:] + tables[:1]):
            got = probe.block_scan(nt, np.stack([u32(a), u32(b)]))
            for call, vals in ((0, a), (1, b)):
                incl = np.cumsum(vals)
                same(got[2 * call], u32((incl - vals) & M32), f"block_excl_scan<{nt}>, call {call + 1}: prefix", vals)
                same(got[2 * call + 1], np.full(nt, u32(incl[-1] & M32)), f"block_excl_scan<{nt}>, call {call + 1}: total", vals)


CHECKS = {"alignbit": check_alignbit, "bfe": check_bfe, "bfi": check_bfi, "shl1": check_shl1, "le4_mask": check_le4_mask,
          "unary": check_unary, "sub_sat_min3": check_sub_sat_min3, "cross_lane": check_cross_lane, "mbcnt": check_mbcnt,
          "readfirstlane": check_readfirstlane, "wave_sync": check_wave_sync, "mul_add_rn": check_mul_add_rn, "memory": check_memory,
          "lds_push_tagged": check_lds_push_tagged, "block_excl_scan": check_block_excl_scan}
