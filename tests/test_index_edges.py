"""The contig index and its three lookup forms with chosen keys (tests/index_cases.py) -- under the SIMT mock and on the GPU.

Every other test feeds the index ntHash values or random numbers into a table that is at most half full: probe sequences of one or two
slots, never across the end of the table, never a refuted tag match, never the key that equals the empty marker.  Here the keys are
crafted for their home slot and tag byte:
  a. one home, clusters of 7 .. 40 keys (past the eight tags of one load, on slot by slot)      e. keys inserted 2, 3 and 200 times
  b. the same across the end of the table, first empty slot exactly 0 and exactly 7              f. record counts on both sides of a resize; no records
  c. clusters that carry only the tag 0x01 or only 0xFF, beside empty slots                      g. contig ids above 65535
  d. the all-ones key absent, once, twice, three times, alone; the key 0
and every case goes through the lookup that reads the tags first (a fresh index) and through the one that reads the slots directly (after
a batch that found all of its minimizers); the lookups inside the emit kernels see an index crafted round the minimizers of random reads.
Conditions of every case: index size == the oracle's; records == the oracle's; n_index_hits == the read minimizers the oracle's index
holds == the hit records, more than none and fewer than all (the inputs are built so that every found key survives the map's filters)."""
import os
import re

import numpy as np
import pytest

import index_cases as ic
import parity_cases as pc
from ntlink_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ntlink_amd", "csrc")
K = ic.K


# ---------------------------------------------------------------- the restatement against the sources

def _squeezed(name):
    return re.sub(r"\s+", " ", open(os.path.join(CSRC, name)).read())


def test_source_literals():
    """keys_at() crafts homes and tags from index_cases.home / tag / table_bits.  If the kernels' multiplier, tag expression or sizing
    rule changes, the crafted clusters quietly turn into scattered keys and the cases above test nothing: change tests/index_cases.py
    with them."""
    common, kernels, host = _squeezed("index_common.h"), _squeezed("map_kernels.h"), _squeezed("ntl_hip.hip")
    assert "uint64_t index_home(uint64_t key, int bits) { return (key * 0x%Xull) >> (64 - bits); }" % ic.MULT in common
    assert "uint8_t index_tag(uint64_t key) { return (uint8_t)(((key >> 20) & 0xFEu) | 1u); }" in common
    assert "int bits = 10; while (((uint64_t)1 << bits) < 2 * ctg->count + 2) bits++; ix->bits = bits; ix->nslots = (uint64_t)1 << bits;" in host
    # the insert and the tag pass use the same two functions (and nothing of their own), and the probe sequence is linear
    assert "uint64_t s = index_home(R.hash, bits);" in kernels and "s = (s + 1) & mask;" in kernels
    assert "four |= (uint32_t)index_tag(key) << (8 * j);" in kernels
    assert len(re.findall(r"0x9E3779B97F4A7C15", common + kernels + host, re.I)) == 1
    assert "if (R.hash == NTL_INF) {" in kernels and "if (key == NTL_INF) return;" in common
    # ... and the restatement itself
    assert (ic.MULT * ic.INV) & ic.M64 == 1
    assert [ic.table_bits(n) for n in (0, 1, 511, 512, 1023, 1024, 2047, 2048)] == [10, 10, 10, 11, 11, 12, 12, 13]
    assert ic.home(0, 10) == 0 and ic.tag(0) == 1 and ic.tag(0xFFFFFFF) == 0xFF and ic.tag(1 << 20) == 1 and ic.tag(1 << 21) == 3


def test_keys_at():
    rng = np.random.default_rng(1)
    for bits, slot, t in ((10, 0, None), (10, 1023, 0x01), (11, 2047, 0xFF), (12, 1234, 0x5B), (20, 77, None)):
        keys = ic.keys_at(slot, bits, 9, rng, tag=t)
        assert len(set(keys)) == 9 and ic.ALL_ONES not in keys
        assert all(ic.home(key, bits) == slot and 0 <= key <= ic.M64 and (t is None or ic.tag(key) == t) for key in keys)
    more = ic.keys_at(5, 10, 4, rng, avoid=keys)
    assert not set(more) & set(keys)
    assert ic.occupied(ic.keys_at(1022, 10, 4, rng), 10) == {1022, 1023, 0, 1} and ic.first_empty({1023, 0}, 1023, 10) == 1


# ---------------------------------------------------------------- the checks (one set for the mock and the GPU)

def _map_arrays(dev, ix, arrays, **kw):
    roff, rlen, rh, rp, rs = arrays
    with dev.sketch_from_arrays(roff, rh, rp, rs) as rsk, dev.map(ix, rsk, rlen, k=K, **kw) as res:
        return res.download(), res.n_index_hits  # (asking for the result stores the batch's hit fraction in the index)


def saturate(dev, ix, all_hit):
    """a batch in which every lookup hits: whatever is made or mapped for this index next looks its keys up in the slots directly"""
    got, nhit = _map_arrays(dev, ix, all_hit)
    assert nhit == len(all_hit[2]) == len(got["hits"]) > 0, "the batch of present keys alone"


def assert_lookups(got, nhit, exp, found, form, name):
    try:
        pc.assert_same_records(got, exp)
    except AssertionError as e:
        raise AssertionError(f"{name}, {form}: {e}") from None
    assert nhit == found, f"{name}, {form}: n_index_hits {nhit}, the oracle's index holds {found} of the read minimizers"
    assert len(got["hits"]) == found, f"{name}, {form}: {len(got['hits'])} hit records for {found} found keys"


def check_array_case(dev, name, direct=True):
    case = ic.array_case(name)
    exp, size, found = case.expected()
    with dev.sketch_from_arrays(case.coff, case.ch, case.cp, case.cs) as csk, dev.index(csk, case.ctg_len) as ix:
        assert len(ix) == size, f"{name}: index size {len(ix)}, oracle {size}"
        got, nhit = _map_arrays(dev, ix, case.reads)  # the first batch on a fresh index: tags first
        assert_lookups(got, nhit, exp, found, "tags first", name)
        if not case.stored:  # no minimizers: no records, and no batch can hit
            assert size == 0 and found == 0 and not len(got["maps"]) and not len(got["hits"]) and not len(got["pafs"])
            return
        assert 0 < found < len(case.reads[2])
        if direct:
            saturate(dev, ix, case.all_hit)
            got, nhit = _map_arrays(dev, ix, case.reads)
            assert_lookups(got, nhit, exp, found, "direct", name)
    dev.sync()


EMIT_FORMS = {"records": {}, "made-for-index": {"index": True}, "for-map-only": {"index": True, "records": False}}


def check_emit_case(dev, w, forms=tuple(EMIT_FORMS), phases=("tags first", "direct")):
    """probe_kernel over the records of a plain sketch, and the lookups inside emit_list_kernel (w = 100: per-strip lists) and emit_kernel
    (w = 40: the bitmask) of a sketch made for the index, with and without records -- each on a fresh index's hit fraction (PROBE == 1)
    and right after a batch that hit throughout (PROBE == 2)."""
    ec = ic.emit_case(w)
    qoff, qh, qp, qs = ec.sketch
    name = f"emit-w{w}"
    with dev.sketch_from_arrays(ec.coff, ec.ch, ec.cp, ec.cs) as csk, dev.index(csk, ec.ctg_len) as ix, dev.batch(ec.seqs) as rb:
        assert len(ix) == ec.index_size
        for phase in phases:
            for form in forms:
                kw = dict(EMIT_FORMS[form])
                if kw.pop("index", False):
                    kw["index"] = ix
                if phase == "direct":
                    saturate(dev, ix, ec.all_hit)  # before the sketch is queued: the emit kernel's form is chosen there
                with dev.sketch(rb, K, w, **kw) as sk, dev.map(ix, sk, ec.rlen, k=K) as res:
                    got, nhit = res.download(), res.n_index_hits
                    assert sk.count == len(qh) and sk.from_lists == (w == 100)
                    if sk.has_records:
                        off, h, p, s = sk.download()
                        assert np.array_equal(off, qoff) and np.array_equal(h, qh) and np.array_equal(p, qp) and np.array_equal(s, qs), \
                            f"{name}, {form}, {phase}: the sketch's records differ from the oracle's"
                assert_lookups(got, nhit, ec.exp, ec.found, f"{form}, {phase}", name)
    dev.sync()


ALL_CASES = list(ic.ARRAY_CASES)
# The mock pays 1 .. 3 s per index + three maps and 3 s per sketch of 20-kb reads (the two emit-time tests: 34 s and 27 s; the 25 tests
# of its half: 43 s of wall time on seven workers on their own).  Its half keeps every letter and every lookup form and drops
# repetitions of one branch: clusters of 8, 10 and 16 (7, 9 and 40 stay: inside the eight tags, the first slot behind them,
# far behind them), four of the nine wrap clusters, the all-ones key three times (twice stays), the record counts 512 and 1023 (both
# sides of 1024 -> 2048 stay with 511 | 1024).  The GPU half runs everything.
SIM_SKIP = {"a-8", "a-10", "a-16", "b-10-at-1021", "b-16-at-1018", "b-9-at-1017", "b-12-at-1022", "d-three-times-across-contigs", "f-512", "f-1023"}
SIM_CASES = [n for n in ALL_CASES if n not in SIM_SKIP]


def test_cases_cover_the_issue():
    letters = {n[0] for n in SIM_CASES}
    assert letters == set("abcdefg") and set(SIM_SKIP) <= set(ALL_CASES) and len(ALL_CASES) == 30


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    d = simlib.device()
    yield d
    d.close()


@pytest.mark.parametrize("name", SIM_CASES)
def test_sim_index_case(sim_dev, name):
    check_array_case(sim_dev, name)


def test_sim_emit_lookups_lists(sim_dev):
    check_emit_case(sim_dev, 100)


def test_sim_emit_lookups_bitmask(sim_dev):
    check_emit_case(sim_dev, 40, forms=("made-for-index", "for-map-only"))


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    d = capi.Device(0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_CASES)
def test_gpu_index_case(gpu_dev, name):
    check_array_case(gpu_dev, name)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [100, 40])
def test_gpu_emit_lookups(gpu_dev, w):
    check_emit_case(gpu_dev, w)
