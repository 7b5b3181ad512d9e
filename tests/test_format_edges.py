"""The text of .verbose_mapping.tsv and .paf from crafted map results (tests/format_cases.py) -- under the SIMT mock and on the GPU, the
same checks.  The records go to the device as they are (Device.mapres_from_host, ntl_mapres_from_host): nothing is mapped.

Every other test formats what the mapper made of small fixtures: positions of five or six digits, hit regions where the gather put
them.  Here:
  digits      every value on both sides of every power of ten, 2^31 and 2^32 - 1 in every field of a hit and of a PAF line, every span
  hit-counts  mappings of 1 .. 1000 hits round a block of 256 threads, regions 0, 1, 63, 64 and 300 slots apart, the first not at slot 0
  shape-*     no record at all; 1 and 257 hits; 255, 256, 257 mappings; no PAF record; grids sized by the PAF records and by the hits
  names       names of 0, 1, 15, 16, 17 and 255 bytes, multi-byte UTF-8, a space
  random      700 mappings, 400 PAF records, every number with a random digit count
  all-max     every number 2^32 - 1 and every name 255 bytes, against the bounds ntl_mapres_format computes, and NTL_FORMAT_MAX_TEXT
For every batch, by byte and array equality: the counts and the download == the dense restatement (NumPy, format_cases); the device's
two texts, their sizes, the rewritten mappings and the ends == the oracle's plain integer formatting of the dense records; either text
alone; the host writers' bytes == the same text.  The digit batch's text goes through formats.read_verbose, too (ntl_vmap's number
parser up to 4294967295).  The refusals of ntl_mapres_from_host, and that of ntl_mapres_gap_cuts for such a result, with their
messages.  Out::u64's pieces of nine digits, which neither text reaches, through ntl_write_indexlr's hashes.

Mapping n_hits cannot take ten digits in a test (it is the number of hits that are there): its one to four digits are in hit-counts."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import format_cases as fc
from helpers import assert_reader_blocks, parsed_verbose_arrays
from ntlink_amd import capi, formats

M32 = fc.M32


def test_cases_cover_the_issue():
    assert fc.V == sorted(set(fc.V)) and len(fc.V) == 22 and fc.V[:5] == [0, 9, 10, 99, 100] and fc.V[-4:] == [10 ** 9, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
    assert list(fc.BATCHES) == ["digits", "hit-counts"] + ["shape-" + s for s in fc.SHAPES] + ["names", "random", "all-max"]
    for name in fc.BATCHES:  # the builders' own assertions run here, without a device
        b = fc.batch(name)
        assert len(b.dense["hits"]) <= 10000 and len(b.dense["hits"]) == int(b.maps["n_hits"].sum())
    assert len(fc.batch("shape-empty").maps) == 0 and len(fc.batch("shape-empty").slots) > 0
    assert len(fc.batch("shape-600-pafs").pafs) == 600 and len(fc.batch("shape-5000-hits").dense["hits"]) == 5000
    # the reference formatting itself, on one record by hand
    b = fc.batch("shape-one-mapping-one-hit")
    h, m = b.dense["hits"][0], b.maps[0]
    assert b.text()[0].decode() == f"rd{m['read']}\tcg{m['ctg']}\t1\t{h['ctg_pos']}:{'-+'[h['ctg_strand']]}_{h['read_pos']}:{'-+'[h['read_strand']]}\n"
    assert fc.batch("all-max").text()[1].split(b"\n")[0] == b"\t".join([b"r" * 255, b"4294967295", b"4294967295", b"4294967295", b"-", b"C" * 255] +
                                                                        [b"4294967295"] * 4 + [b"0", b"255"])


def test_host_writer_splits_64_bit_values_at_1e9():
    """Out::u64 prints a value above 2^32 - 1 in pieces of nine digits.  Neither text here reaches that: the one 64-bit number of a PAF
    line is t_end - t_start of two 32-bit numbers.  The minimizer hashes of ntl_write_indexlr do, so the pieces are held to plain
    integer formatting there: low pieces of 0, 1, 8, 9 digits (the zeros in front must be printed), two and three pieces, the
    largest value."""
    e9 = 10 ** 9
    lows = [0, 1, 9, 10, 99999999, 100000000, 999999999]
    hashes = [M32, M32 + 1, M32 + 2] + [k * e9 + lo for k in (5, 4294967, 4294967296, 18446744073) for lo in lows if k * e9 + lo > M32]
    hashes += [10 ** 18, 10 ** 18 + 1, 10 ** 19, 2 ** 63, (4294967296 * e9 + 7) * e9 + 5, 2 ** 64 - e9, 2 ** 64 - 1]
    hashes = [h for h in hashes if h < 2 ** 64]
    assert sum(1 for h in hashes if h >= M32 * e9 + e9) >= 4, "three pieces"
    h = np.array(hashes, np.uint64)
    pos = np.array([fc.V[i % len(fc.V)] for i in range(len(h))], np.uint32)
    strand = (np.arange(len(h)) % 2).astype(np.uint8)
    off = np.array([0, 3, 3, len(h)], np.uint64)
    with tempfile.TemporaryFile("w+b") as fh:
        formats.write_indexlr(fh, ["a", "none", "b"], [7, 0, 2 ** 32 - 1], off, h, pos, strand, True)
        fh.seek(0)
        got = fh.read().decode()
    toks = [f"{hashes[i]}:{int(pos[i])}:{'-+'[strand[i]]}" for i in range(len(h))]
    assert got == f"a\t7\t{' '.join(toks[:3])}\nnone\t0\t\nb\t4294967295\t{' '.join(toks[3:])}\n"


# ---------------------------------------------------------------- the checks (the same for the mock and the GPU)

def _host_text(b):
    """the host writers (ntl_write_verbose / ntl_write_paf) over the dense records"""
    with tempfile.TemporaryFile("w+b") as fv, tempfile.TemporaryFile("w+b") as fp:
        formats.write_verbose(fv, b.dense, b.read_names, b.ctg_names)
        formats.write_paf(fp, b.dense, b.read_names, b.read_len, b.ctg_names, b.ctg_len)
        fv.seek(0); fp.seek(0)
        return fv.read(), fp.read()


def _download_text(dev, txt):
    d = txt.download()
    out = bytes(d["verbose"]), bytes(d["paf"]), d["maps"].copy(), d["ends"].copy()
    dev.pinned_release(d["_pinned"])
    return out


def check_batch(dev, name, tmp_path=None):
    b = fc.batch(name)
    exp_v, exp_p = b.text()
    dm, dh, dp = b.dense["maps"], b.dense["hits"], b.dense["pafs"]
    first = dh[dm["hit_off"].astype(np.int64)]
    last = dh[(dm["hit_off"] + dm["n_hits"] - 1).astype(np.int64)]
    with dev.mapres_from_host(b.maps, b.slots, b.pafs) as res, dev.names(b.read_names, b.read_len) as rn, dev.names(b.ctg_names, b.ctg_len) as cn:
        assert isinstance(res, capi.MapResult)
        # 1. counts and the dense copy
        assert res.counts() == (len(dm), len(dh), len(dp)), name
        assert res.n_index_hits == 0
        rec = res.download()
        assert np.array_equal(rec["maps"], dm), f"{name}: the mappings with hit_off in the dense numbering"
        assert np.array_equal(rec["hits"], dh), f"{name}: the hits gathered from their regions"
        assert np.array_equal(rec["pafs"], dp), name
        # 2. the device's text
        with res.format(rn, cn, True, True) as txt:
            sizes = txt.sizes()
            got_v, got_p, maps, ends = _download_text(dev, txt)
        assert (len(got_v), len(got_p)) == (len(exp_v), len(exp_p)), f"{name}: {len(got_v)}, {len(got_p)} bytes of text, the oracle has {len(exp_v)}, {len(exp_p)}"
        assert got_v == exp_v, f"{name}: verbose text, first difference at byte {next(i for i in range(len(exp_v)) if got_v[i] != exp_v[i])}"
        assert got_p == exp_p, f"{name}: PAF text, first difference at byte {next(i for i in range(len(exp_p)) if got_p[i] != exp_p[i])}"
        assert sizes == (len(exp_v), len(exp_p), len(dm)), name
        assert np.array_equal(maps, dm) and np.array_equal(ends[0::2], first) and np.array_equal(ends[1::2], last), name
        with res.format(rn, cn, False, True) as txt:
            assert txt.sizes() == (0, len(exp_p), len(dm))
            v, p, maps, ends = _download_text(dev, txt)
        assert v == b"" and p == exp_p and np.array_equal(maps, dm) and np.array_equal(ends[0::2], first) and np.array_equal(ends[1::2], last), name
        with res.format(rn, cn, True, False) as txt:
            assert txt.sizes() == (len(exp_v), 0, len(dm))
            v, p, maps, ends = _download_text(dev, txt)
        assert v == exp_v and p == b"" and np.array_equal(maps, dm) and np.array_equal(ends[0::2], first) and np.array_equal(ends[1::2], last), name
        # the dense copy is the same behind the formatter (it shares the dense offsets)
        again = res.download()
        assert np.array_equal(again["maps"], dm) and np.array_equal(again["hits"], dh)
        if name == "all-max":
            check_bounds(dev, b, res, rn, cn)
    dev.sync()
    # 3. the host writers
    host_v, host_p = _host_text(b)
    assert host_v == exp_v, f"{name}: ntl_write_verbose"
    assert host_p == exp_p, f"{name}: ntl_write_paf"
    # 4. the digit batch through the reader
    if tmp_path is not None:
        path = str(tmp_path / "digits.verbose_mapping.tsv")
        with open(path, "wb") as fh:
            fh.write(got_v)
        want = parsed_verbose_arrays(path, b.ctg_names)
        assert len(want[2]) == len(dm) and np.array_equal(want[4], dh) and want[2]["ctg"].tolist() == dm["ctg"].tolist()
        for max_bytes in (0, 300):
            assert_reader_blocks(list(formats.read_verbose(path, b.ctg_names, max_bytes=max_bytes, lib_path=dev.lib_path)), want)


def check_bounds(dev, b, res, rn, cn):
    """the longest text stays below what ntl_mapres_format allows for it; NTL_FORMAT_MAX_TEXT at that bound refuses, one above makes
    the same bytes"""
    exp_v, exp_p = b.text()
    vb, pb = fc.verbose_bound(len(b.dense["hits"]), len(b.maps), b.names2), fc.paf_bound(len(b.pafs), b.names2)
    assert len(exp_v) < vb and len(exp_p) < pb, (len(exp_v), vb, len(exp_p), pb)
    assert "NTL_FORMAT_MAX_TEXT" not in os.environ
    try:
        os.environ["NTL_FORMAT_MAX_TEXT"] = str(vb)
        with pytest.raises(capi.NtlError, match="may exceed 4 GB") as ei:
            res.format(rn, cn, True, True)
        assert ei.value.code == capi.NTL_ERANGE
        os.environ["NTL_FORMAT_MAX_TEXT"] = str(vb + 1)
        with res.format(rn, cn, True, True) as txt:
            got_v, got_p, _maps, _ends = _download_text(dev, txt)
        assert got_v == exp_v and got_p == exp_p
    finally:
        del os.environ["NTL_FORMAT_MAX_TEXT"]


def check_refusals(dev):
    """what ntl_mapres_from_host refuses, with its messages; what it accepts at the edges; ntl_mapres_gap_cuts on its result"""
    hit = (5, 6, 1, 0, (0, 0))
    slots = np.array([hit] * 10, capi.HIT_DT)
    none = np.zeros(0, capi.PAF_DT)

    def maps(*regions):
        return np.array([(0, 0, n, 0, off) for off, n in regions], capi.MAPPING_DT)
    for regions, message in [
            ([(0, 2), (2, 0), (2, 3)], "mapping 1 has no hits"),
            ([(0, 2), (8, 3)], "mapping 1 leaves hit_slots"),
            ([(11, 1)], "mapping 0 leaves hit_slots"),
            ([(0, 2), (2 ** 40, 1)], "mapping 1 leaves hit_slots"),
            ([(0, 4), (3, 2)], "mapping 1 overlaps or lies in front of the one before it"),
            ([(4, 2), (0, 2)], "mapping 1 overlaps or lies in front of the one before it"),
            ([(0, 2), (4, 2), (4, 2)], "mapping 2 overlaps or lies in front of the one before it")]:
        with pytest.raises(capi.NtlError, match=message) as ei:
            dev.mapres_from_host(maps(*regions), slots, none)
        assert ei.value.code == capi.NTL_EINVAL, regions
    # null arrays with non-zero counts: the binding never passes them, so the C entry itself
    m, q = maps((0, 2)), np.zeros(1, capi.PAF_DT)
    for args in [(None, 1, slots.ctypes.data, 10, None, 0), (m.ctypes.data, 1, None, 10, None, 0), (m.ctypes.data, 1, slots.ctypes.data, 10, None, 1)]:
        p = C.c_void_p()
        assert dev.L.ntl_mapres_from_host(dev.ptr, *args, C.byref(p)) == capi.NTL_EINVAL and not p.value
        assert "a null array with a non-zero count" in dev.L.ntl_last_error(dev.ptr).decode()
    # accepted: regions that touch, the last one up to the last slot; PAF records alone; nothing at all
    for mm, ss, qq, counts in [(maps((0, 2), (2, 3), (5, 5)), slots, none, (3, 10, 0)), (maps(), slots[:0], q, (0, 0, 1)), (maps(), slots[:0], none, (0, 0, 0))]:
        with dev.mapres_from_host(mm, ss, qq) as res:
            assert res.counts() == counts
    # ntl_mapres_gap_cuts reads map_off, which only a grouped result has: an error code, not a read
    with dev.mapres_from_host(maps((1, 2), (4, 2)), slots, none) as res:
        with pytest.raises(capi.NtlError, match="ntl_mapres_gap_cuts: not a result of ntl_map_run_grouped") as ei:
            res.gap_cuts([0, 1], [1, 0], 20)
        assert ei.value.code == capi.NTL_EINVAL
        with pytest.raises(capi.NtlError):
            res.grouped_info
        assert res.counts() == (2, 4, 0)  # ... and the result is still good
    dev.sync()


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    d = simlib.device()
    yield d
    d.close()


@pytest.mark.parametrize("name", list(fc.BATCHES))
def test_sim_format_batch(sim_dev, name, tmp_path):
    check_batch(sim_dev, name, tmp_path if name == "digits" else None)


def test_sim_from_host_refusals(sim_dev):
    check_refusals(sim_dev)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    d = capi.Device(0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(fc.BATCHES))
def test_gpu_format_batch(gpu_dev, name, tmp_path):
    check_batch(gpu_dev, name, tmp_path if name == "digits" else None)


@pytest.mark.gpu
def test_gpu_from_host_refusals(gpu_dev):
    check_refusals(gpu_dev)
