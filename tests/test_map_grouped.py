"""Grouped mapping (Device.map_grouped -> ntl_map_run_grouped, csrc/group_kernels.h): every read looked up in the contigs of its own group
only -- under the SIMT mock and on the GPU, the same checks (tests/group_cases.py builds the inputs and what the oracle makes of every
group on its own).
  a. the same key in two groups: found in both            e. clusters of 9 and 20 keys of one home, a cluster across the table's end
  b. a key twice in one group: dropped there only         f. n = S/2 - 2, S/2 - 1, S/2, 3 S: both sides of the LDS / global threshold
  c. group A's keys asked for by group B's reads          g. no groups; groups without contigs, reads, minimizers
  d. the all-ones key absent / once / twice; the key 0    h. contig numbers above 65535
Conditions of every case: records == the oracle's, group by group, numbers shifted to the global ones; n_index_hits == the oracle's sum
== the hit records, more than none and fewer than all read minimizers; groups_in_lds / groups_in_global == the sizing rule's."""
import os
import re

import numpy as np
import pytest

import group_cases as gc
import index_cases as ic
import parity_cases as pc
from ntlink_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = gc.K


def test_source_literals():
    """group_cases crafts homes from index_cases.home / table_bits: the grouped kernel must size and address its tables the same way"""
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "ntlink_amd", "csrc", "group_kernels.h")).read())
    assert "#define GROUP_MIN_BITS 10 " in src
    assert "int bits = GROUP_MIN_BITS; while (((uint64_t)1 << bits) < 2ull * n + 2ull) bits++; return bits;" in src
    assert src.count("index_home(") == 2 and "s = (s + 1u) & mask;" in src and "0x9E37" not in src
    # the probe loops are bounded by the table's slot count (a wrong size is an error, not a hang)
    assert src.count("if (step == nslots) { atomicOr(A.err, GROUP_ERR_PROBE); break; }") == 2


# ---------------------------------------------------------------- the checks (one set for the mock and the GPU)

def run_grouped(dev, comp, **kw):
    """(records, n_index_hits, grouped_info); the sketches and every array are gone before the result is read"""
    args = dict(comp.kw)
    args.update(kw)
    csk = dev.sketch_from_arrays(comp.coff, comp.ch, comp.cp, comp.cs)
    rsk = dev.sketch_from_arrays(comp.roff, comp.rh, comp.rp, comp.rs)
    res = dev.map_grouped(csk, comp.ctg_len.copy(), comp.cgo.copy(), rsk, comp.rlen.copy(), comp.rgo.copy(), **args)
    csk.close(); rsk.close()
    with res:
        return res.download(), res.n_index_hits, res.grouped_info


def check_composite(dev, comp, partial=True):
    got, nhit, info = run_grouped(dev, comp)
    try:
        pc.assert_same_records(got, comp.exp)
    except AssertionError as e:
        raise AssertionError(f"{comp.name}: {e}") from None
    assert nhit == comp.found, f"{comp.name}: n_index_hits {nhit}, the oracle's indexes hold {comp.found} of the read minimizers"
    if partial:
        assert len(got["hits"]) == comp.found, f"{comp.name}: {len(got['hits'])} hit records for {comp.found} found keys"
        assert 0 < comp.found < len(comp.rh), comp.name
    in_lds, in_global = comp.expected_info(info["lds_slots"])
    assert (info["groups_in_lds"], info["groups_in_global"]) == (in_lds, in_global), (comp.name, info)
    dev.sync()
    return info


def check_crafted(dev, name, arg=None):
    return check_composite(dev, gc.crafted(name, arg))


def check_sizes(dev):
    """f: S comes from the library; both kinds of table must have been used"""
    S = lds_slots(dev)
    info = check_crafted(dev, "f", S)
    assert info["groups_in_lds"] == 3 and info["groups_in_global"] == 2


def lds_slots(dev):
    comp = gc.crafted("a")
    with dev.sketch_from_arrays(comp.coff, comp.ch, comp.cp, comp.cs) as csk, dev.sketch_from_arrays(comp.roff, comp.rh, comp.rp, comp.rs) as rsk, \
            dev.map_grouped(csk, comp.ctg_len, comp.cgo, rsk, comp.rlen, comp.rgo, k=K) as res:
        S = res.grouped_info["lds_slots"]
    assert S >= 1024 and S & (S - 1) == 0 and S * 16 <= 64 * 1024
    return S


def check_no_groups(dev):
    empty = np.zeros(1, np.uint64)
    none = (np.empty(0, np.uint64), np.empty(0, np.uint32), np.empty(0, np.uint8))
    with dev.sketch_from_arrays(empty, *none) as csk, dev.sketch_from_arrays(empty, *none) as rsk, \
            dev.map_grouped(csk, np.empty(0, np.uint32), np.zeros(1, np.uint32), rsk, np.empty(0, np.uint32), np.zeros(1, np.uint32), k=K) as res:
        assert res.counts() == (0, 0, 0) and res.n_index_hits == 0
        assert res.grouped_info["groups_in_lds"] == 0 and res.grouped_info["groups_in_global"] == 0


def check_ordinary_result_has_no_info(dev):
    case = ic.array_case("a-7")
    with dev.sketch_from_arrays(case.coff, case.ch, case.cp, case.cs) as csk, dev.index(csk, case.ctg_len) as ix, \
            dev.sketch_from_arrays(*[case.reads[i] for i in (0, 2, 3, 4)]) as rsk, dev.map(ix, rsk, case.reads[1], k=K) as res:
        with pytest.raises(capi.NtlError) as e:
            res.grouped_info
        assert e.value.code == capi.NTL_EINVAL


def check_argument_errors(dev):
    comp = gc.crafted("a")

    def refused(cgo, rgo, csk, rsk):
        with pytest.raises(capi.NtlError) as e:
            dev.map_grouped(csk, comp.ctg_len, cgo, rsk, comp.rlen, rgo, k=K)
        assert e.value.code == capi.NTL_EINVAL and len(str(e.value)) > len("error -1: "), str(e.value)

    with dev.sketch_from_arrays(comp.coff, comp.ch, comp.cp, comp.cs) as csk, dev.sketch_from_arrays(comp.roff, comp.rh, comp.rp, comp.rs) as rsk:
        down = comp.cgo.copy(); down[1] = down[2] + 1  # offsets that decrease
        refused(down, comp.rgo, csk, rsk)
        down = comp.rgo.copy(); down[1] = down[2] + 1
        refused(comp.cgo, down, csk, rsk)
        short = comp.cgo.copy(); short[-1] -= 1        # offsets that do not end at nseq
        refused(short, comp.rgo, csk, rsk)
        short = comp.rgo.copy(); short[-1] -= 1
        refused(comp.cgo, short, csk, rsk)
        late = comp.rgo.copy(); late[0] = 1            # ... or do not start at 0
        refused(comp.cgo, late, csk, rsk)
        # a sketch made only to be mapped against one index holds no records
        case = ic.array_case("a-7")
        rng = np.random.default_rng(5)
        seqs = [bytes(gc.ACGT[rng.integers(0, 4, 300)]) for _ in range(len(comp.rlen))]
        with dev.sketch_from_arrays(case.coff, case.ch, case.cp, case.cs) as isk, dev.index(isk, case.ctg_len) as ix, dev.batch(seqs) as rb, \
                dev.sketch(rb, K, 10, index=ix, records=False) as for_map:
            refused(comp.cgo, comp.rgo, csk, for_map)
    dev.sync()


def check_random(dev, n_groups, k, w, n_single=32):
    comp = gc.random_case(n_groups, k, w)
    got, nhit, info = run_grouped(dev, comp)
    pc.assert_same_records(got, comp.exp)
    assert nhit == comp.found and 0 < nhit < len(comp.rh)
    assert len(got["maps"]) > n_groups // 4, "the reads are cut from their group's contigs: most of them map"
    assert (info["groups_in_lds"], info["groups_in_global"]) == comp.expected_info(info["lds_slots"])
    assert info["groups_in_lds"] > 0 and info["groups_in_global"] >= n_groups // 10
    # ... and the existing index + map, one group at a time, gives the grouped result's slice
    picked = [g for g in range(n_groups) if comp.rgo[g + 1] > comp.rgo[g]][:n_single]
    for g in picked:
        grp = comp.groups[g]
        roff, rlen, rh, rp, rs = grp.reads
        with dev.sketch_from_arrays(grp.coff, grp.ch, grp.cp, grp.cs) as csk, dev.index(csk, grp.ctg_len) as ix, \
                dev.sketch_from_arrays(roff, rh, rp, rs) as rsk, dev.map(ix, rsk, rlen, **comp.kw) as res:
            one = res.download()
        r0, r1, c0 = int(comp.rgo[g]), int(comp.rgo[g + 1]), int(comp.cgo[g])
        sel = (got["maps"]["read"] >= r0) & (got["maps"]["read"] < r1)
        m = got["maps"][sel].copy()
        assert len(m) == len(one["maps"]), f"group {g}"
        if len(m):
            h0 = int(m["hit_off"][0])
            m["read"] -= r0; m["ctg"] -= c0; m["hit_off"] -= h0
            assert m.tobytes() == one["maps"].tobytes(), f"group {g}: mappings"
            assert got["hits"][h0:h0 + len(one["hits"])].tobytes() == one["hits"].tobytes(), f"group {g}: hits"
        p = got["pafs"][(got["pafs"]["read"] >= r0) & (got["pafs"]["read"] < r1)].copy()
        p["read"] -= r0; p["ctg"] -= c0
        assert p.tobytes() == one["pafs"].tobytes(), f"group {g}: PAF records"
    dev.sync()


def check_lifetime(dev):
    """the inputs go right after the call; two grouped results and an ordinary one queued back to back, read in reverse order"""
    a, b = gc.crafted("b"), gc.crafted("e")
    single_a, _, _ = run_grouped(dev, a)
    single_b, _, _ = run_grouped(dev, b)
    case = ic.array_case("a-9")
    roff, rlen, rh, rp, rs = case.reads

    def queue(comp):
        csk = dev.sketch_from_arrays(comp.coff, comp.ch, comp.cp, comp.cs)
        rsk = dev.sketch_from_arrays(comp.roff, comp.rh, comp.rp, comp.rs)
        arrays = [comp.ctg_len.copy(), comp.cgo.copy(), comp.rlen.copy(), comp.rgo.copy()]
        res = dev.map_grouped(csk, arrays[0], arrays[1], rsk, arrays[2], arrays[3], **comp.kw)
        csk.close(); rsk.close()
        for arr in arrays:
            arr[:] = 0xFFFFFFF  # the caller's arrays are free again
        del arrays
        return res

    with dev.sketch_from_arrays(case.coff, case.ch, case.cp, case.cs) as csk, dev.index(csk, case.ctg_len) as ix, \
            dev.sketch_from_arrays(roff, rh, rp, rs) as rsk:
        with dev.map(ix, rsk, rlen, k=K) as res:
            single_o = res.download()
        ra = queue(a)
        rb = queue(b)
        ro = dev.map(ix, rsk, rlen, k=K)
    for res, single in ((ro, single_o), (rb, single_b), (ra, single_a)):  # in reverse order
        with res:
            pc.assert_same_records(res.download(), single)
    pc.assert_same_records(single_a, a.exp)
    pc.assert_same_records(single_b, b.exp)
    dev.sync()


CRAFTED = ["a", "b", "c", "d", "e", "g"]
N_EMPTY = {"sim": 300, "gpu": 66000}  # h: groups between the two with records (the mock pays three barriers of 256 threads per group)


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    dev = simlib.device()
    yield dev
    dev.close()


@pytest.mark.parametrize("name", CRAFTED)
def test_sim_crafted(sim_dev, name):
    check_crafted(sim_dev, name)


def test_sim_sizes(sim_dev):
    check_sizes(sim_dev)


def test_sim_contig_ids(sim_dev):
    check_crafted(sim_dev, "h", N_EMPTY["sim"])


def test_sim_no_groups(sim_dev):
    check_no_groups(sim_dev)
    check_ordinary_result_has_no_info(sim_dev)


def test_sim_argument_errors(sim_dev):
    check_argument_errors(sim_dev)


@pytest.mark.parametrize("k,w", [(20, 10), (15, 5)])
def test_sim_random(sim_dev, k, w):
    check_random(sim_dev, 60, k, w, n_single=8)


def test_sim_lifetime(sim_dev):
    check_lifetime(sim_dev)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    dev = capi.Device(0)
    yield dev
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CRAFTED)
def test_gpu_crafted(gpu_dev, name):
    check_crafted(gpu_dev, name)


@pytest.mark.gpu
def test_gpu_sizes(gpu_dev):
    check_sizes(gpu_dev)


@pytest.mark.gpu
def test_gpu_contig_ids(gpu_dev):
    check_crafted(gpu_dev, "h", N_EMPTY["gpu"])


@pytest.mark.gpu
def test_gpu_no_groups(gpu_dev):
    check_no_groups(gpu_dev)
    check_ordinary_result_has_no_info(gpu_dev)


@pytest.mark.gpu
def test_gpu_argument_errors(gpu_dev):
    check_argument_errors(gpu_dev)


@pytest.mark.gpu
@pytest.mark.parametrize("k,w", [(20, 10), (15, 5)])
def test_gpu_random(gpu_dev, k, w):
    check_random(gpu_dev, 500, k, w)


@pytest.mark.gpu
def test_gpu_lifetime(gpu_dev):
    check_lifetime(gpu_dev)
