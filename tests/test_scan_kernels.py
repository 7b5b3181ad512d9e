"""The exclusive scans that size every variable-length output (csrc/scan_kernels.h) against np.cumsum in uint64, reduced mod 2^32,
under the SIMT mock and on the GPU, the same checks.  The probe (tests/probe) calls scan_launch -- the launch sequence device_scan
itself calls -- with the product's SCAN_SELF_MAX_TILES, and with 0, which takes the three-launch path (scan_reduce_kernel +
scan_tiles_kernel + scan_down_kernel: n > 8 388 608 in the product) at a small n; and scan_tiles_kernel alone, in place, as the emit
stage launches it, over more than one SCAN_TILE of words (its carry loop).  Every comparison is exact."""
import functools

import numpy as np
import pytest

from probe import probelib
from probe.probelib import FILL

LAUNCH_N = (0, 1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4096, 4097, 3 * 2048 + 5)
TILES_N = (0, 1, 2047, 2048, 2049, 4097, 6000)
KINDS = ("zero", "one", "random", "ones32")
SLOT = 0x0BADF00D  # what an input array holds in its entry n, the place of the sum: no kernel may read it as an item


@functools.lru_cache(maxsize=None)
def items(kind, n, row):
    """row `row` of a batch whose first row is of `kind`: the rows of a batch differ in kind, the random ones in their seed"""
    kind = KINDS[(KINDS.index(kind) + row) % len(KINDS)]
    if kind == "random":
        v = np.random.default_rng(1000 * row + n).integers(0, 1 << 20, n, dtype=np.uint64)
    else:
        v = np.full(n, {"zero": 0, "one": 1, "ones32": 0xFFFFFFFF}[kind], np.uint64)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def reference(kind, n, row):
    """(the exclusive scan mod 2^32, the sum mod 2^32) of items(kind, n, row): computed once, shared"""
    v = items(kind, n, row)
    incl = np.cumsum(v, dtype=np.uint64)
    excl = ((incl - v) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    excl.setflags(write=False)
    return excl, int(incl[-1]) & 0xFFFFFFFF if n else 0


MODES = ((True, False), (True, True), (False, False), (False, True))  # (in == out, sums_dev given)


def check_launch(probe, three_launches, batch, every_mode):
    """both paths of scan_launch: arrays at stride n + 1 with the sum at [n], in place and not, with and without the sums' array.
    every_mode: all four MODES for every (n, kind), which the GPU does in milliseconds; else one of them in turn, so that every n and
    every kind still meets all four (the mock starts a thread per lane for every launch)"""
    self_max = 0 if three_launches else probe.self_max_tiles
    assert probe.self_max_tiles == 4096 and probe.scan_tile == 2048
    for n in LAUNCH_N:
        tiles = probe.tile_count(n)
        assert tiles == max(1, -(-n // 2048)) and (tiles > self_max) == three_launches
        for kind in KINDS:
            data = np.concatenate([np.append(items(kind, n, y).astype(np.uint32), np.uint32(SLOT)) for y in range(batch)])
            want = np.concatenate([np.append(reference(kind, n, y)[0], np.uint32(reference(kind, n, y)[1])) for y in range(batch)])
            totals = [reference(kind, n, y)[1] for y in range(batch)]
            if n >= 2 and kind == "ones32":
                assert totals[0] == (-n) & 0xFFFFFFFF  # the sum wrapped
            turn = (LAUNCH_N.index(n) + KINDS.index(kind)) % 4
            for inplace, with_sums in (MODES if every_mode else MODES[turn:turn + 1]):
                what = f"n={n} batch={batch} {kind} {'in == out' if inplace else 'in != out'} sums_dev {'given' if with_sums else 'null'}"
                out, back, sums, tile = probe.scan(data, n, batch, inplace, with_sums, self_max)
                bad = np.flatnonzero(out[:want.size] != want)
                assert bad.size == 0, f"{what}: out differs at {bad[:8].tolist()} (array, index: {[divmod(int(b), n + 1) for b in bad[:8]]}): " \
                                      f"{out[bad[:8]].tolist()}, the reference has {want[bad[:8]].tolist()}"
                assert (out[want.size:] == FILL).all(), f"{what}: the words behind the last out[n] changed"
                if not inplace:
                    assert (back == data).all(), f"{what}: the input changed"
                if with_sums:
                    assert sums[:batch].tolist() == totals and sums[:batch].tolist() == [int(out[y * (n + 1) + n]) for y in range(batch)], what
                    assert sums[batch] == FILL, f"{what}: the word behind the sums changed"
                assert (tile[tiles * batch:] == FILL).all(), f"{what}: the tile buffer changed behind tiles x batch"


def check_tiles_kernel(probe):
    """scan_tiles_kernel alone and in place: gridDim.y arrays of n words side by side, the totals at total_stride apart"""
    for n in TILES_N:
        for gy in (1, 2):
            for kind in KINDS:
                data = np.concatenate([items(kind, n, y).astype(np.uint32) for y in range(gy)]) if n else np.zeros(0, np.uint32)
                want = np.concatenate([reference(kind, n, y)[0] for y in range(gy)]) if n else np.zeros(0, np.uint32)
                totals = [reference(kind, n, y)[1] for y in range(gy)]
                for stride in (0, n + 1):
                    for with_extra in (False, True):
                        what = f"n={n} gridDim.y={gy} {kind} total_stride={stride} extra {'given' if with_extra else 'null'}"
                        buf, total, extra = probe.scan_tiles(data, n, gy, stride, with_extra)
                        bad = np.flatnonzero(buf[:want.size] != want)
                        assert bad.size == 0, f"{what}: data differs at {bad[:8].tolist()}: {buf[bad[:8]].tolist()}, the reference has {want[bad[:8]].tolist()}"
                        assert (buf[want.size:] == FILL).all(), f"{what}: the words behind the data changed"
                        if stride:
                            assert [int(total[y * stride]) for y in range(gy)] == totals, what
                            rest = np.delete(total, [y * stride for y in range(gy)])
                        else:  # every array's total goes to the one word (the product launches gridDim.y = 1 this way): one of them stays
                            assert int(total[0]) in totals, what
                            rest = total[1:]
                        assert (rest == FILL).all(), f"{what}: words beside the totals changed"
                        if with_extra:
                            assert extra[:gy].tolist() == totals and extra[gy] == FILL, what


PATHS = pytest.mark.parametrize("three_launches", [False, True], ids=["self", "tiles_down"])
BATCH = pytest.mark.parametrize("batch", [1, 3])


@pytest.fixture(scope="module")
def sim_probe():
    return probelib.probe("sim")


@pytest.fixture(scope="module")
def gpu_probe():
    return probelib.probe("gpu")


@PATHS
@BATCH
def test_sim_scan_launch(sim_probe, three_launches, batch):
    check_launch(sim_probe, three_launches, batch, every_mode=False)


def test_sim_scan_tiles_kernel(sim_probe):
    check_tiles_kernel(sim_probe)


@pytest.mark.gpu
@PATHS
@BATCH
def test_gpu_scan_launch(gpu_probe, three_launches, batch):
    check_launch(gpu_probe, three_launches, batch, every_mode=True)


@pytest.mark.gpu
def test_gpu_scan_tiles_kernel(gpu_probe):
    check_tiles_kernel(gpu_probe)
