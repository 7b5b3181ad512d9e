"""One strip length per sketch (window_plan): 4096 ordinals, or -- NTL_SKETCH_STRIP=8192, for the windows of sketch_wave_kernel's
large-window shape (w >= 235 at ten candidates per window, k <= 64) -- 8192, where a lane of the wave kernel holds 128 k-mers and every
pass behind it runs on strips of 512 lanes.  The same reads are sketched with both lengths and every minimizer is compared with the
oracle -- under the SIMT mock and on the GPU."""
import numpy as np
import pytest

import parity_cases as pc

K, W = 32, 250
LONG = 8192                       # ordinals of a long strip
NWO = (512 - ((W - 16) // 16 + 2)) * 16 - 1   # windows a long strip owns at w = 250: 7935
_rnd = pc.random_bases


def _of_kmers(rng, m, k=K):
    """a random sequence of m k-mers"""
    return pc.of_kmers(rng, m, k)


def boundary_reads(rng):
    """Lengths, in k-mers, that straddle 8192 - w, 8192 and 2 * 8192, and the seams of the long strips' own windows (a read of
    NWO + w - 1 k-mers fills one strip's windows exactly; one more starts a second strip)."""
    ms = [LONG - W - 1, LONG - W, LONG - W + 1, LONG - 1, LONG, LONG + 1, 2 * LONG - 1, 2 * LONG, 2 * LONG + 1,
          NWO + W - 2, NWO + W - 1, NWO + W, 2 * NWO + W - 1, 2 * NWO + W, W - 1, W, W + 1]
    return [_of_kmers(rng, m) for m in ms]


def tail_reads(rng):
    """A sequence's last strip rolls the multiple of 16 k-mers per lane that covers it, 16 .. 128: first strips (element 0 is
    virtual: m + 1 elements) that end just below, at and just above every multiple of 1024 elements, and second strips (they start
    at ordinal NWO - 1) of 16, 48, 80 and 128 k-mers per lane."""
    out = [_of_kmers(rng, 1024 * j + d) for j in range(1, 9) for d in (-2, -1, 0) if 1024 * j + d >= W]
    out += [_of_kmers(rng, NWO - 1 + 1024 * j + d) for j in (1, 3, 5, 8) for d in (-1, 0, 1)]
    return out


special_reads = pc.special_reads


def both_lengths(dev, monkeypatch, seqs, k=K, w=W):
    """check_sketch with the knob at 4096 and at 8192; the runs' strip statistics"""
    st = {}
    for strip in (4096, 8192):
        with monkeypatch.context() as m:
            m.setenv("NTL_SKETCH_STRIP", str(strip))
            info = {}
            pc.check_sketch(dev, seqs, k, w, info=info)
            st[strip] = info
    return st


def check_geometries(dev, monkeypatch):
    rng = np.random.default_rng(8192)
    reads = boundary_reads(rng) + tail_reads(rng)
    st = both_lengths(dev, monkeypatch, reads)
    # the knob took: the long geometry cuts the same reads into fewer strips (n windows: ceil(n / 7935) against ceil(n / 3839))
    nwin = [len(s) - K + 1 - W + 1 for s in reads]
    assert st[8192]["strips"] == sum(-(-n // NWO) for n in nwin if n > 0), st
    assert st[4096]["strips"] == sum(-(-n // 3839) for n in nwin if n > 0), st
    assert st[4096]["from_lists"] and st[8192]["from_lists"]
    withn, lowc = special_reads(rng)
    both_lengths(dev, monkeypatch, withn)
    st = both_lengths(dev, monkeypatch, lowc)
    assert st[8192]["redo_strips"] > 0 and st[4096]["redo_strips"] > 0, st
    # every strip through all three passes, and most strips through the block-minima pass behind the wave kernel
    with monkeypatch.context() as m:
        m.setenv("NTL_SKETCH_FORCE_REDO", "1")
        st = both_lengths(dev, monkeypatch, reads[:12] + withn)
        assert st[8192]["fallback_strips"] == st[8192]["redo_strips"] > 0, st
    with monkeypatch.context() as m:
        m.setenv("NTL_SKETCH_THRESH", "4")
        st = both_lengths(dev, monkeypatch, reads[:12])
        assert st[8192]["fallback_strips"] > 3, st
    # the large windows (two range-minimum levels in the block-minima pass), another k, and the bitmask instead of the lists
    both_lengths(dev, monkeypatch, reads[:9] + lowc[:1], k=40, w=600)
    both_lengths(dev, monkeypatch, reads[3:12], k=21, w=235)
    with monkeypatch.context() as m:
        m.setenv("NTL_SKETCH_LISTS", "0")
        st = both_lengths(dev, monkeypatch, reads[:9] + withn[:1])
        assert not st[8192]["from_lists"]


def check_near_ties(dev, monkeypatch):
    """Two different k-mers whose ring keys the window pass cannot order, the two smallest of one window of 240: whichever length the
    strips have, each such sequence (one strip) goes to the exact pass and comes out as the oracle's."""
    k, w = 16, 240
    seqs = pc.near_tie_sequences(k, 10, flank=125)
    assert all(len(s) - k + 1 >= w for s in seqs)
    st = both_lengths(dev, monkeypatch, seqs, k=k, w=w)
    for strip in (4096, 8192):
        assert st[strip]["redo_strips"] == st[strip]["strips"] == len(seqs), (strip, st)


def given_up_share(dev, monkeypatch, strip, nbases, nreads):
    rng = np.random.default_rng(250)
    seqs = [_rnd(rng, nbases // nreads) for _ in range(nreads)]
    with monkeypatch.context() as m:
        m.setenv("NTL_SKETCH_STRIP", str(strip))
        info = {}
        pc.check_sketch(dev, seqs, K, W, info=info)
    share = info["fallback_strips"] / info["strips"]
    print(f"strips of {strip}: {info['fallback_strips']} of {info['strips']} given up by the wave kernel ({100 * share:.2f} %), "
          f"{info['redo_strips']} to the exact pass")
    return share, info


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    d = simlib.device()
    yield d
    d.close()


def test_sim_strip_geometries_match_oracle(sim_dev, monkeypatch):
    check_geometries(sim_dev, monkeypatch)


def test_sim_strip_geometries_near_ties(sim_dev, monkeypatch):
    check_near_ties(sim_dev, monkeypatch)


def test_sim_default_geometry_follows_the_plan(sim_dev, monkeypatch):
    """No knob: the plan's own choice still sketches right, and windows outside the long strips' range ignore the knob."""
    rng = np.random.default_rng(7)
    reads = [_of_kmers(rng, m) for m in (LONG + 1, 3000, NWO + W)]
    info = {}
    pc.check_sketch(sim_dev, reads, K, W, info=info)
    monkeypatch.setenv("NTL_SKETCH_STRIP", "8192")
    pc.check_sketch(sim_dev, reads, K, 100, info=info)
    nwin = [len(s) - K + 1 - 100 + 1 for s in reads]
    assert info["strips"] == sum(-(-n // ((256 - 7) * 16 - 1)) for n in nwin), info


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    from ntlink_amd import capi
    d = capi.Device(0)
    yield d
    d.close()


@pytest.mark.gpu
def test_gpu_strip_geometries_match_oracle(gpu_dev, monkeypatch):
    check_geometries(gpu_dev, monkeypatch)


@pytest.mark.gpu
def test_gpu_strip_geometries_near_ties(gpu_dev, monkeypatch):
    check_near_ties(gpu_dev, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("strip", [4096, 8192])
def test_gpu_wave_kernel_gives_up_few_strips(gpu_dev, monkeypatch, strip):
    """The passes behind the wave kernel must not hide a broken fast path: on random sequence at w = 250 it gives up at most 2 % of
    its strips.  Expected: a strip is given up, above all, for a window without a candidate -- a gap of w between two of its
    40960 / w candidates per 4096 k-mers, 0.96^250 = 3.7e-5 each: 0.6 % of the strips of 4096 (0.7 % measured), 1.2 % of those of
    8192 -- so 60 Mbases (9000 strips of 8192, sigma 0.12 %) tell 1.3 % from 2 %; the few hundred strips the mock can afford would
    not, so the share is asserted here only.  Measured: 0.67 % of 18000 strips of 4096, 1.20 % of 9000 strips of 8192."""
    share, info = given_up_share(gpu_dev, monkeypatch, strip, 60_000_000, 3000)
    assert info["strips"] > 7000
    assert share <= 0.02, (share, info)
