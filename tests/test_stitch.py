"""Resident bytes and the stitch (Device.ascii / Device.stitch -> ntl_ascii_create / ntl_stitch, csrc/stitch_kernels.h) against plain
Python -- slicing, bytes.translate with the reference's table (bin/ntlink_patch_gaps.py:50-53) and .lower() -- under the SIMT mock and
on the GPU, the same checks.
  a. crafted segment lists: every small length and the lengths around the tile, every source and output alignment, many segments in
     one lane's 16 bytes, pieces over one and two tile boundaries, all 256 byte values under every flag, LOWER_FIRST on empty and
     one-byte pieces, fills, one record named a hundred times, two and three stores, no segment at all
  b. 300 random segments over ten random sources with lower case, N runs and IUPAC codes
  c. the ranged copy in three uneven pieces; NTL_EINVAL with a message for every refusal; a store destroyed right after the stitch
     was queued"""
import functools

import numpy as np
import pytest

from ntlink_amd import capi
from ntlink_amd.capi import NTL_STITCH_FILL as FILL, NTL_STITCH_LOWER as LOWER, NTL_STITCH_LOWER_FIRST as FIRST, NTL_STITCH_REVCOMP as REV

T = 16384  # STITCH_TILE of csrc/stitch_kernels.h
TABLE = bytes.maketrans(b"ACGTUNMRWSYKVHDBacgtunmrwsykvhdb", b"TGCAANKYWSRMBDHVtgcaankywsrmbdhv")
ALPHABET = np.frombuffer(b"ACGTACGTACGTacgtNnRYKMSWBDHVryu", np.uint8)
LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 3)
FLAGS = (0, REV, LOWER, REV | LOWER, FIRST, REV | FIRST)


def rand(rng, n):
    return ALPHABET[rng.integers(0, len(ALPHABET), n)].tobytes()


def piece(stores, seg):
    """one segment in plain Python"""
    store, rec, lo, hi, flags = seg
    if store == FILL:
        return bytes([rec]) * (hi - lo)
    out = stores[store][rec][lo:hi]
    if flags & REV:
        out = out[::-1].translate(TABLE)
    if flags & LOWER:
        out = out.lower()
    if flags & FIRST:
        out = out[:1].lower() + out[1:]
    return out


def expected(stores, segs):
    return b"".join(piece(stores, s) for s in segs)


@functools.lru_cache(maxsize=None)
def crafted():
    """(stores, {case name: segment list}) -- the cases share three stores"""
    rng = np.random.default_rng(11)
    every = bytes(range(256))
    long = rand(rng, 3 * T + 100)
    s0 = [long, every, rand(rng, 300), b"", rand(rng, 1)]
    s1 = [rand(rng, n) for n in (40, 41, 1, 2, 777)] + [rand(rng, 1) for _ in range(40)]
    s2 = [b">scaffold_1\n", b">ntLink_0\n", rand(rng, 90)]
    cases = {}
    # every length, forward and reversed, from an odd source offset, behind an odd output offset
    cases["lengths"] = [(FILL, ord("N"), 0, 3, 0)] + [(0, 0, 5, 5 + n, f) for n in LENGTHS for f in (0, REV)]
    # source lo at every residue 0..17 (forward, reversed, lower-cased)
    cases["source_residues"] = [(0, 0, r, r + 100 + r, f) for r in range(18) for f in (0, REV, REV | LOWER)]
    # the output start at every residue mod 16: r fill bytes in front, a total that is no multiple of 16
    for r in range(16):
        cases[f"output_residue_{r}"] = [(FILL, ord("\n"), 0, r, 0), (0, 0, 7, 7 + 200, 0), (0, 0, 9, 9 + 77, REV), (0, 2, 0, 300, LOWER),
                                        (FILL, ord("N"), 0, 16 - r + 5, 0)]
        assert len(expected((s0,), cases[f"output_residue_{r}"])) % 16 != 0
    # 40 one-byte segments from different records with empty segments between them: many segments in one lane's 16 bytes
    tiny = []
    for i in range(40):
        tiny += [(1, 5 + i, 0, 1, (0, REV, LOWER, FIRST)[i % 4]), (1, 0, 7, 7, REV), (0, 3, 0, 0, 0), (FILL, ord("N"), 4, 4, 0)]
    cases["one_byte_segments"] = [(0, 2, 0, 5, 0)] + tiny + [(0, 2, 0, 9, 0)]
    # a piece over one and over two tile boundaries, forward and reversed
    for f in (0, REV):
        cases[f"one_boundary_{f}"] = [(FILL, ord("N"), 0, T - 100, 0), (0, 0, 3, 3 + 300, f), (1, 4, 0, 777, f)]
        cases[f"two_boundaries_{f}"] = [(0, 2, 0, 123, f), (0, 0, 1, 1 + 2 * T + 50, f), (0, 2, 1, 18, f)]
    # all 256 byte values under every flag, whole and from the middle
    cases["all_bytes"] = [(0, 1, lo, hi, f) for f in FLAGS + (LOWER | FIRST, REV | LOWER | FIRST) for lo, hi in ((0, 256), (60, 100), (65, 66))]
    # LOWER_FIRST on pieces of length 0 and 1: behind an empty one the NEXT piece's first byte stays as it is
    up = next(i for i, c in enumerate(long) if i >= 30 and 65 <= c <= 90)
    cases["lower_first"] = [(0, 0, up, up, FIRST), (0, 0, up, up + 20, 0), (0, 0, up, up + 1, FIRST), (0, 0, up, up + 1, 0),
                            (0, 0, up, up, REV | FIRST), (0, 0, up - 19, up + 1, REV), (0, 0, up - 19, up + 1, REV | FIRST),
                            (0, 3, 0, 0, FIRST), (0, 1, 65, 70, 0)]
    got = expected((s0,), cases["lower_first"])
    assert got[0] == long[up] and got[20] == long[up] + 32 and got[21] == long[up]
    # fills of N and of the newline with lengths 0, 1 and T + 1
    cases["fills"] = [(FILL, b, 0, n, 0) for n in (0, 1, T + 1) for b in (ord("N"), ord("\n"))] + [(FILL, ord("N"), 1000, 1017, 0)]
    # one record named by 100 segments
    cases["one_record_100"] = [(0, 2, i, i + 1 + (7 * i) % 150, (0, REV, LOWER, FIRST)[i % 4]) for i in range(100)]
    # two and three stores; header lines from a small store
    cases["two_stores"] = [(1, 0, 0, 40, 0), (0, 2, 10, 200, REV), (1, 1, 0, 41, LOWER), (0, 4, 0, 1, 0)]
    cases["three_stores"] = [(2, 0, 0, 12, 0), (0, 2, 0, 300, 0), (FILL, ord("N"), 0, 20, 0), (1, 4, 700, 777, REV | LOWER), (2, 2, 0, 90, FIRST),
                             (FILL, ord("\n"), 0, 1, 0), (2, 1, 0, 10, 0), (1, 4, 0, 777, REV), (FILL, ord("\n"), 0, 1, 0)]
    cases["nothing"] = []
    cases["only_empty"] = [(0, 0, 4, 4, REV), (FILL, ord("N"), 9, 9, 0)]
    return (s0, s1, s2), cases


@functools.lru_cache(maxsize=None)
def random_case(seed=2024, n=300):
    rng = np.random.default_rng(seed)
    sources = []
    for _ in range(10):
        seq = bytearray(rand(rng, int(rng.integers(1, 3000))))
        for _run in range(int(rng.integers(0, 5))):
            a = int(rng.integers(0, len(seq)))
            b = min(len(seq), a + int(rng.integers(1, 60)))
            seq[a:b] = b"N" * (b - a)
        sources.append(bytes(seq))
    stores = (sources[:6], sources[6:])
    segs = []
    for _ in range(n):
        if rng.random() < 0.15:
            segs.append((FILL, int(rng.choice([78, 10, 110])), 0, int(rng.integers(0, 70)), 0))
            continue
        st = int(rng.integers(0, 2))
        rec = int(rng.integers(0, len(stores[st])))
        lo, hi = sorted(rng.integers(0, len(stores[st][rec]) + 1, 2).tolist())
        if rng.random() < 0.3:
            hi = min(hi, lo + int(rng.integers(0, 20)))
        segs.append((st, rec, lo, hi, int(rng.integers(0, 8))))
    return stores, segs


@functools.lru_cache(maxsize=None)
def reference(which):
    """the expected text of every case: computed once, shared"""
    if which == "random":
        stores, segs = random_case()
        return expected(stores, segs)
    stores, cases = crafted()
    return {name: expected(stores, segs) for name, segs in cases.items()}


def stitch(dev, stores, segs):
    with dev.stitch(stores, segs) as st:
        got = st.download().tobytes()
        assert st.nbytes == len(got)
    return got


def check_crafted(dev):
    host, cases = crafted()
    want = reference("crafted")
    stores = [dev.ascii(recs) for recs in host]
    assert [s.nrec for s in stores] == [len(recs) for recs in host] and stores[0].nbytes == sum(len(r) for r in host[0])
    for name, segs in cases.items():
        got = stitch(dev, stores, segs)
        assert len(got) == len(want[name]), name
        if got != want[name]:
            at = next(i for i, (a, b) in enumerate(zip(got, want[name])) if a != b)
            raise AssertionError(f"{name}: byte {at} of {len(got)}: {got[max(0, at - 8):at + 8]!r}, expected {want[name][max(0, at - 8):at + 8]!r}")
    assert want["nothing"] == b"" and want["only_empty"] == b"" and len(want["lengths"]) > 8 * T
    # one store alone, given as a buffer with offsets that do not start at 0
    buf = np.frombuffer(b"xx" + b"".join(host[2]), np.uint8)
    off = 2 + np.concatenate([[0], np.cumsum([len(r) for r in host[2]])])
    with dev.ascii(buf, off) as alone:
        assert stitch(dev, [alone], [(0, 2, 5, 60, REV), (0, 0, 0, 12, 0)]) == expected((host[2],), [(0, 2, 5, 60, REV), (0, 0, 0, 12, 0)])
    for s in stores:
        s.close()
    dev.sync()


def check_random(dev):
    host, segs = random_case()
    stores = [dev.ascii(recs) for recs in host]
    want = reference("random")
    assert stitch(dev, stores, np.array(segs, capi.STITCH_SEG_DT)) == want
    # the ranged copy in three uneven pieces equals the whole
    with dev.stitch(stores, segs) as st:
        n = st.nbytes
        cuts = [0, 1, n // 3 + 5, n]
        buf = dev.pinned_empty(n)
        parts = [st.copy(a, b, buf).tobytes() for a, b in zip(cuts, cuts[1:])]
        dev.pinned_release(buf)
        assert b"".join(parts) == want
        assert st.copy(7, 7, np.empty(1, np.uint8)).tobytes() == b""
        with pytest.raises(capi.NtlError) as e:
            st.copy(0, n + 1, np.empty(n + 1, np.uint8))
        assert e.value.code == capi.NTL_EINVAL and "outside the result" in str(e.value)
    for s in stores:
        s.close()
    dev.sync()


def check_refusals(dev):
    host, _cases = crafted()
    a, b = dev.ascii(host[0]), dev.ascii(host[2])
    for segs, text in (([(2, 0, 0, 1, 0)], "store 2 out of range"), ([(0, 0, 0, 1, 0), (1, 3, 0, 0, 0)], "segment 1: record 3 out of range"),
                       ([(0, 2, 5, 4, 0)], "lo 5 is above hi 4"), ([(0, 2, 0, 301, 0)], "beyond the record's 300 bytes"),
                       ([(0, 2, 0, 3, 8)], "unknown flag bits"), ([(FILL, 78, 0, 3, REV)], "a fill takes no flags"),
                       ([(FILL, 78, 3, 2, 0)], "lo 3 is above hi 2"), ([(FILL, 256, 0, 2, 0)], "is no byte")):
        with pytest.raises(capi.NtlError) as e:
            dev.stitch([a, b], segs)
        assert e.value.code == capi.NTL_EINVAL and text in str(e.value), str(e.value)
    with pytest.raises(capi.NtlError):
        dev.ascii(np.zeros(4, np.uint8), [0, 3, 2])
    # a store destroyed right after the stitch was queued
    segs = [(0, 0, 3, 3 + 2 * T, REV), (1, 2, 0, 90, 0)]
    st = dev.stitch([a, b], segs)
    a.close()
    b.close()
    assert st.download().tobytes() == expected((host[0], host[2]), segs)
    st.close()
    dev.sync()


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    dev = simlib.device()
    yield dev
    dev.close()


def test_sim_crafted(sim_dev):
    check_crafted(sim_dev)


def test_sim_random(sim_dev):
    check_random(sim_dev)


def test_sim_refusals(sim_dev):
    check_refusals(sim_dev)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    dev = capi.Device(0)
    yield dev
    dev.close()


@pytest.mark.gpu
def test_gpu_crafted(gpu_dev):
    check_crafted(gpu_dev)


@pytest.mark.gpu
def test_gpu_random(gpu_dev):
    check_random(gpu_dev)


@pytest.mark.gpu
def test_gpu_refusals(gpu_dev):
    check_refusals(gpu_dev)
