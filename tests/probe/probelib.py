"""Builds and opens the probe of the instruction wrappers and the scan kernels (intrin_probe.hip, test tool): the same source
with hipcc for gfx950 over ntlink_amd/csrc/dev_intrin.h ("gpu") and with g++ over the SIMT mock's file of that name ("sim")."""
import ctypes
import os
import subprocess

import numpy as np

from ntlink_amd import build as product_build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "build")
CSRC = os.path.join(ROOT, "ntlink_amd", "csrc")
SIM = os.path.join(ROOT, "tests", "sim")
PROBE = os.path.join(HERE, "intrin_probe.hip")
HEADERS = [os.path.join(CSRC, f) for f in ("dev_common.h", "dev_intrin.h", "scan_kernels.h")]
SRC = {"gpu": [PROBE] + HEADERS,
       "sim": [PROBE] + HEADERS[:1] + HEADERS[2:] + [os.path.join(SIM, "sim_runtime.cpp"), os.path.join(SIM, "include", "dev_intrin.h"),
                                                     os.path.join(SIM, "include", "hip", "hip_runtime.h")]}
LIB = {"gpu": os.path.join(OUT, "libintrin_probe_hip.so"), "sim": os.path.join(OUT, "libintrin_probe_sim.so")}

# the operations of probe_kernel, in the order of its enum
OPS = ("alignbit", "bfe", "bfi", "shl1_or_ne", "shl1_or_le", "shl1_or_eq", "shl1_or_lt_diff", "le4_mask", "row_min16", "row_max16",
       "quad_min", "quad_sum", "wave_min", "wave_incl_scan", "mbcnt", "brev", "double", "sub_sat", "min3", "mul_add_rn", "load_u64_a1",
       "load_u32_a1", "store_u64_a1", "load4_a4", "stream", "lds_load2_ordered", "lds_push_tagged", "wave_sync", "readfirstlane")
ALL_LANES = (1 << 64) - 1
FILL = 0xA5A5A5A5  # what an output table holds before the probe runs


def command(kind, out):
    if kind == "gpu":  # the product's flags (ntlink_amd/build.py), one step
        return [product_build.hipcc_path(), *product_build._flags(), "-shared", "-I", CSRC, PROBE, "-o", out]
    # the SIMT mock's flags and include order (tests/sim/simlib.py)
    return ["g++", "-O1", "-g1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wall",
            "-Wno-unused-function", "-Wno-unknown-pragmas", "-x", "c++",
            "-I", os.path.join(SIM, "include"), "-I", CSRC, PROBE, os.path.join(SIM, "sim_runtime.cpp"), "-o", out]


def build(kind):
    """Serialised across processes (pytest-xdist workers): a file lock around the build; rebuilt when a source is newer."""
    import fcntl
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        out = LIB[kind]
        if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in SRC[kind])):
            subprocess.check_call(command(kind, out))
        return out


def _u32(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


class Probe:
    def __init__(self, kind):
        self.kind = kind
        lib = self.lib = ctypes.CDLL(build(kind))
        u32p, u64, u32, i = ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        lib.probe_run.argtypes = [i, i, u32p, u64, u32p, u64, u32, ctypes.c_ulonglong]
        lib.probe_block_scan.argtypes = [u32, u32p, u32p]
        lib.probe_scan.argtypes = [u32p, u32p, u32p, u64, u64, u32, i, u32p, u64, u64, u32p, u64]
        lib.probe_scan_tiles.argtypes = [u32p, u64, u64, u32, u32p, u64, u64, u32p, u64]
        for f in (lib.probe_scan_tile_count, lib.probe_scan_self_max_tiles):
            f.restype = u64
        lib.probe_scan_tile_count.argtypes = [u64]
        lib.probe_scan_tile.restype = u32
        assert lib.probe_op_count() == len(OPS)
        self.push_t = lib.probe_push_t()
        self.scan_tile = lib.probe_scan_tile()
        self.self_max_tiles = lib.probe_scan_self_max_tiles()

    def tile_count(self, n):
        return self.lib.probe_scan_tile_count(n)

    def run(self, op, table, out_words, nthreads=256, param=0, active=ALL_LANES):
        """`table`: the input table, any integer or float64 array (taken as its 32-bit words); returns the output table, u32[out_words]"""
        words = np.ascontiguousarray(table).view(np.uint32).ravel().copy()
        out = np.full(out_words, FILL, np.uint32)
        rc = self.lib.probe_run(OPS.index(op), param, _u32(words), words.size, _u32(out), out.size, nthreads, active)
        assert rc == 0, f"probe_run({op}) returned {rc}"
        return out

    def block_scan(self, nt, table):
        words = np.ascontiguousarray(table, np.uint32).ravel().copy()
        assert words.size == 2 * nt
        out = np.full(4 * nt, FILL, np.uint32)
        rc = self.lib.probe_block_scan(nt, _u32(words), _u32(out))
        assert rc == 0, f"probe_block_scan({nt}) returned {rc}"
        return out.reshape(4, nt)

    def scan(self, data, n, batch, inplace, with_sums, self_max_tiles, guard=4):
        """data: u32[batch * (n + 1)].  Returns (out with `guard` words behind it, the input array afterwards or None, sums with one word
        behind them or None, the tile buffer with `guard` words behind tiles * batch)"""
        data = np.ascontiguousarray(data, np.uint32)
        assert data.size == batch * (n + 1)
        out = np.full(data.size + guard, FILL, np.uint32)
        if inplace:
            out[:data.size] = data
        src, back = data.copy(), np.full(data.size, FILL, np.uint32)
        sums = np.full(batch + 1, FILL, np.uint32) if with_sums else None
        tile = np.full(self.tile_count(n) * batch + guard, FILL, np.uint32)
        rc = self.lib.probe_scan(None if inplace else _u32(src), None if inplace else _u32(back), _u32(out), guard, n, batch, int(inplace),
                                 _u32(sums) if with_sums else None, batch + 1 if with_sums else 0, self_max_tiles, _u32(tile), tile.size)
        assert rc == 0, f"probe_scan returned {rc}"
        return out, None if inplace else back, sums, tile

    def scan_tiles(self, data, n, gy, total_stride, with_extra, guard=4):
        """data: u32[gy * n].  Returns (data with `guard` words behind it, the totals' array with one word behind the last total, extra
        with one word behind it or None)"""
        buf = np.full(gy * n + guard, FILL, np.uint32)
        buf[:gy * n] = data
        total = np.full((gy - 1) * total_stride + 2, FILL, np.uint32)
        extra = np.full(gy + 1, FILL, np.uint32) if with_extra else None
        rc = self.lib.probe_scan_tiles(_u32(buf), buf.size, n, gy, _u32(total), total_stride, total.size,
                                       _u32(extra) if with_extra else None, gy + 1 if with_extra else 0)
        assert rc == 0, f"probe_scan_tiles returned {rc}"
        return buf, total, extra


_open = {}


def probe(kind):
    """one build and one load per process and kind"""
    if kind not in _open:
        _open[kind] = Probe(kind)
    return _open[kind]
