"""The overlap stage's filter (ntl_overlap_filter: ovl_insert_kernel, ovl_resolve_kernel, the scan, ovl_gather_kernel) with chosen keys
(tests/overlap_cases.py) -- under the SIMT mock and on the GPU, the same checks.

Every other test feeds the filter ntHash values of real or random sequence: sub-tables at most half full, probe sequences of one or two
slots, never across the end of a sequence's own slots, never the key that equals the empty marker.  Here:
  1. clusters of 3, 9 and 40 keys of one high word at the last slot of a sub-table (they wrap to its slot 0) and in its middle, keys of
     them inserted 2, 3 and 200 times                                   5. records on and beside the ends of their regions, position 0
  2. the same keys once each in the sequences in front and behind,         and 2^32 - 1, overlapping regions, none, a duplicate outside
  3. the key 2^64 - 1 absent, once, twice, three times, once outside,   6. 255, 256, 257 records; a sequence boundary at record 256;
     alone, in adjacent sequences; the keys 0 and 0xFFFFFFFF00000000       5000 records in 300 sequences, 300 records in 2500
  4. sequences of 0, 1 and 2 records, empty ones first and last,        7. 300 random sequences of keys from 8 high words x 16 low words
     a batch of no sequences, a batch of no records                        and the all-ones key
Offsets, hashes, positions and strands must equal the oracle's (the strands: the input's at the oracle's kept records); integers, no
tolerance.  The conditions of the cases -- what each sequence keeps, how many clusters cross the end of their sub-table -- are asserted
in overlap_cases on the oracle's output and a linear-probe simulation, never on the product's."""
import os
import re

import numpy as np
import pytest

import overlap_cases as oc
from ntlink_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ntlink_amd", "csrc")


# ---------------------------------------------------------------- the restatement against the source

def test_source_literals():
    """overlap_cases crafts its clusters from overlap_cases.home and the layout of the sub-tables.  If the kernels' home function, the
    sub-table's place or the probe rule changes, the crafted clusters quietly turn into scattered keys and the cases test nothing:
    change tests/overlap_cases.py with them."""
    src = re.sub(r"\s+", " ", open(os.path.join(CSRC, "overlap_kernels.h")).read())
    assert "uint64_t ovl_home(uint64_t key, uint64_t size) { return (uint64_t)(((key >> 32) * size) >> 32);" in src
    # insert and resolve place and walk the sub-table alike: base and size from mx_off, linear, wrapping inside the sub-table
    assert src.count("const uint64_t base = 2ull * A.mx_off[seq], size = 2ull * (A.mx_off[seq + 1] - A.mx_off[seq]);") == 2
    assert src.count("uint64_t j = ovl_home(R.hash, size);") == 2 and src.count("const uint64_t s = base + j;") == 2
    assert src.count("if (++j == size) j = 0;") == 2
    # the all-ones key never enters the table
    assert "if (R.hash == NTL_INF) { atomicAdd(&A.side[seq], 1u); return; }" in src
    assert "if (R.hash == NTL_INF) { A.keep[i] = A.side[seq] == 1u ? 1u : 0u; return; }" in src
    # ... and the restatement itself
    assert oc.home(oc.ALL_ONES - 1, 2) == 1 and oc.home(oc.LAST_ZERO, 600) == 599 and oc.home(0xFF000000 << 32, 600) == 597
    assert oc.home(oc.HW_MID << 32, 600) == 300 and oc.home(0xFFFFFFFF, 600) == 0 and oc.home(1 << 32, 1 << 31) == 0
    a, b, c = oc.LAST_ZERO | 1, oc.LAST_ZERO | 2, oc.LAST_ZERO | 3
    assert oc.probe([a, b, oc.ALL_ONES, a, c], 10) == ({a: 9, b: 0, c: 1}, True) and oc.probe([a, 5], 10) == ({a: 9, 5: 0}, False)


def test_cases_cover_the_issue():
    crafted = oc.batch("crafted")
    names = [s.name for s in crafted.seqs]
    assert {n[0] for n in names} == set("12345") and len(names) == 65 and len(crafted.hash) > 7 * 256
    assert crafted.seqs[0].kind == crafted.seqs[-1].kind == "empty"
    assert list(oc.BATCHES) == ["crafted", "total-255", "total-256", "total-257", "boundary-at-256", "geometry-records", "geometry-offsets",
                                "random-300", "empty-0-sequences", "empty-7-sequences"]
    wrapping, ones = oc.batch("random-300").reach()
    assert wrapping >= 20 and ones >= 20


# ---------------------------------------------------------------- the check (one for the mock and the GPU)

def check_batch(dev, name):
    b = oc.batch(name)
    e_off, eh, ep, es = b.expected()
    with dev.sketch_from_arrays(b.mx_off, b.hash, b.pos, b.strand) as sk:
        assert sk.nseq == len(b.seqs) and sk.count == len(b.hash)
        with dev.overlap_filter(sk, b.reg_off, b.starts, b.ends) as kept:
            assert kept.nseq == len(b.seqs)
            g_off, gh, gp, gs = kept.download()
    dev.sync()
    assert len(g_off) == len(e_off) and int(g_off[-1]) == len(gh) == len(gp) == len(gs), f"{name}: offsets and records of the result do not fit"
    for s, seq in enumerate(b.seqs):  # by sequence, so that a failure names its case
        ga, gb, ea, eb = int(g_off[s]), int(g_off[s + 1]), int(e_off[s]), int(e_off[s + 1])
        got = list(zip(gh[ga:gb].tolist(), gp[ga:gb].tolist(), gs[ga:gb].tolist()))
        want = list(zip(eh[ea:eb].tolist(), ep[ea:eb].tolist(), es[ea:eb].tolist()))
        assert got == want, f"{name}, {seq.name}: {len(got)} records kept of {len(seq.keys)}, the oracle keeps {len(want)}; " \
                            f"only here {sorted(set(got) - set(want))[:4]}, only there {sorted(set(want) - set(got))[:4]}"
    assert np.array_equal(g_off, e_off) and np.array_equal(gh, eh) and np.array_equal(gp, ep) and np.array_equal(gs, es), name


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    d = simlib.device()
    yield d
    d.close()


@pytest.mark.parametrize("name", list(oc.BATCHES))
def test_sim_overlap_batch(sim_dev, name):
    check_batch(sim_dev, name)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    d = capi.Device(0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(oc.BATCHES))
def test_gpu_overlap_batch(gpu_dev, name):
    check_batch(gpu_dev, name)
