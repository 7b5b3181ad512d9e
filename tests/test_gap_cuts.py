"""The cut points of every gap, decided on the device (MapResult.gap_cuts -> ntl_mapres_gap_cuts, csrc/gap_kernels.h) and applied by
ntlink_amd.gapfill.map_long_reads -- under the SIMT mock and on the GPU, the same checks.
  a. golden: map_long_reads against the end state the reference's own map_long_reads leaves (tests/golden/gen/gapcut_cases.json.gz, made
     by tests/golden/gen_goldens_gapcuts.py: every pair's five fields, every scaffold's two cuts), --stringent off and on, in one batch
     and in batches of a few gaps
  b. random gaps: MapResult.gap_cuts == a restatement of bin/ntlink_patch_gaps.py:113-127, 291-308, 492-517 written here, applied to
     res.download() of the same result
  c. NTL_EINVAL for an ordinary result, other group offsets, a wrong n_gaps; a result destroyed right after the call"""
import argparse
import functools
import gzip
import json
import os
import types

import numpy as np
import pytest

import group_cases as gc
import index_cases as ic
from ntlink_amd import capi, gapfill

HERE = os.path.dirname(os.path.abspath(__file__))
K, W = 20, 10
REVCOMP = bytes.maketrans(b"ACGTN", b"TGCAN")


# ---------------------------------------------------------------- a. golden

@functools.lru_cache(maxsize=None)
def golden():
    with gzip.open(os.path.join(HERE, "golden", "gen", "gapcut_cases.json.gz"), "rt") as fh:
        doc = json.load(fh)
    with gzip.open(os.path.join(HERE, "golden", "gen", doc["base"]), "rt") as fh:
        base = json.load(fh)
    doc["scaffolds"] = base["scaffolds"] + doc["scaffolds"]
    doc["reads"] = base["reads"] + doc["reads"]
    n = len(doc["reads"])
    assert n >= 69 and len(doc["scaffolds"]) == 2 * n and len(doc["tags"]) == n and len(doc["preset"]) == n
    assert [s["stringent"] for s in doc["sets"]] == [False, True]
    return doc


def check_golden(dev, tmp_path, stringent, batch_bases=gapfill.BATCH_BASES):
    doc = golden()
    exp = doc["sets"][int(stringent)]
    prefix = str(tmp_path / "g")
    for suffix, recs in ((".scaffolds.masked_temp.fa", doc["scaffolds"]), (".reads.masked_temp.fa", doc["reads"])):
        with open(prefix + suffix, "w") as fh:
            for rid, seq in recs:
                fh.write(f">{rid}\n{seq}\n")
    pairs = {}
    for (rid, _seq), (sc, sr, tc, tr) in zip(doc["reads"], doc["preset"]):
        pairs[tuple(rid.split("__")[1:])] = types.SimpleNamespace(source_ctg_cut=sc, source_read_cut=sr, target_ctg_cut=tc, target_read_cut=tr,
                                                                  old_anchor_used=False)
    scaffolds = {name: types.SimpleNamespace(length=length, five_prime_cut=0, three_prime_cut=length) for name, length in doc["lengths"].items()}
    args = argparse.Namespace(o=prefix, k=doc["k"], w=doc["w"], z=doc["z"], x=doc["x"], sensitive=doc["sensitive"], stringent=stringent)
    gapfill.map_long_reads(pairs, scaffolds, args, dev=dev, batch_bases=batch_bases)
    for g, (p, want, tag) in enumerate(zip(pairs.values(), exp["pairs"], doc["tags"])):
        got = [p.source_ctg_cut, p.source_read_cut, p.target_ctg_cut, p.target_read_cut, p.old_anchor_used]
        assert got == want, f"gap {g} ({tag}), stringent={stringent}: {got}, the reference leaves {want}"
    got = {name: [s.five_prime_cut, s.three_prime_cut] for name, s in scaffolds.items()}
    assert got == exp["scaffolds"]
    # the fixture's own reach: new cuts, fallbacks, and a scaffold cut at both ends
    assert any(w[4] for w in doc["sets"][0]["pairs"]) and not all(w[4] for w in doc["sets"][0]["pairs"])
    assert 0 < exp["scaffolds"]["chB"][0] < exp["scaffolds"]["chB"][1] < doc["lengths"]["chB"]
    dev.sync()


# ---------------------------------------------------------------- b. random gaps

def _flank(rng, n):
    return gc.ACGT[rng.integers(0, 4, n)]


@functools.lru_cache(maxsize=None)
def random_gaps(seed=2025):
    """About 300 gaps: (scaffold sequences, read sequences, src_minus, tgt_minus).  A read is the end of the source flank, some bases of
    its own and the start of the target flank (group_cases' pieces), reverse-complemented at random; the signs are random.  Families
    with error-free reads sweep the target's reach base by base so that the hit counts 1, 2, 63, 64, 65 occur (two minimizers in 11
    bases at w10: 64 hits are about 350 bases); flanks of 1 kb give the counts above 128; the rest are random with 5 % substitutions,
    some without one flank or without either."""
    rng = np.random.default_rng(seed)
    gaps = []

    def gap(src, tgt, reach_s, reach_t, rate):
        parts = [src[len(src) - reach_s:], _flank(rng, int(rng.integers(0, 300))), tgt[:reach_t]]
        read = np.concatenate(parts)
        if rate:
            read = gc._mutate(read, rate, rng)
        if len(read) < K:
            read = _flank(rng, 200)
        gaps.append((src, tgt, read))

    src, tgt = _flank(rng, 400), _flank(rng, 400)
    for reach in range(K, K + 40, 2):          # 0, 1, 2, ... hits on the target
        gap(src, tgt, 300, reach, 0.0)
    src, tgt = _flank(rng, 700), _flank(rng, 700)
    for reach in range(300, 420, 2):           # 63, 64, 65 among them
        gap(src, tgt, 250, reach, 0.0)
    for _ in range(12):                        # above 128
        src, tgt = _flank(rng, 1000), _flank(rng, 1000)
        gap(src, tgt, int(rng.integers(850, 1001)), int(rng.integers(850, 1001)), 0.0)
    LAST = len(gaps) - 1
    for i in range(16):                        # a segment of one 1 kb flank moved (even i) or reverse-complemented (odd i) in the read
        src, tgt = _flank(rng, 1000), _flank(rng, 1000)
        a, b, c = sorted(rng.choice(np.arange(100, 900, 50), 3, replace=False).tolist())
        piece = tgt if i & 2 else src
        if i & 1:
            other = np.concatenate([piece[:a], np.frombuffer(piece[a:b].tobytes().translate(REVCOMP)[::-1], np.uint8), piece[b:]])
        else:
            other = np.concatenate([piece[:a], piece[b:c], piece[a:b], piece[c:]])
        gaps.append((src, tgt, np.concatenate([src if i & 2 else other, _flank(rng, 100), other if i & 2 else tgt])))
    while len(gaps) < 300:
        src, tgt = _flank(rng, int(rng.integers(200, 1001))), _flank(rng, int(rng.integers(200, 1001)))
        kind = rng.random()
        reach_s = 0 if kind < 0.15 else int(rng.integers(60, len(src) + 1))
        reach_t = 0 if 0.1 < kind < 0.25 else int(rng.integers(60, len(tgt) + 1))
        gap(src, tgt, reach_s, reach_t, 0.05)
    gaps = [gaps[i] for i in rng.permutation(len(gaps)) if i != LAST] + [gaps[LAST]]  # one of the 1 kb family stays the last gap
    scaffolds, reads = [], []
    for src, tgt, read in gaps:
        read = read.tobytes()
        if rng.random() < 0.5:
            read = read.translate(REVCOMP)[::-1]
        scaffolds += [src.tobytes(), tgt.tobytes()]
        reads.append(read)
    n = len(reads)
    return scaffolds, reads, rng.integers(0, 2, n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8)


def find_orientation(hits):
    """:113-119"""
    if all(h["ctg_strand"] == h["read_strand"] for h in hits):
        return "+"
    if all(h["ctg_strand"] != h["read_strand"] for h in hits):
        return "-"
    return None


def check_position_consistency(hits):
    """:121-127"""
    return all(a["ctg_pos"] < b["ctg_pos"] for a, b in zip(hits, hits[1:])) or all(a["ctg_pos"] > b["ctg_pos"] for a, b in zip(hits, hits[1:]))


def assign_ctg_cut(position, read_ori, ctg_ori, k):
    """:291-299"""
    return position + k if read_ori == ctg_ori and ctg_ori == "-" else position


def assign_read_cut(position, read_ori, ctg_ori, k):
    """:301-308"""
    return position + k if read_ori != ctg_ori and ctg_ori == "+" else position


def restated(rec, n, src_minus, tgt_minus, k):
    """what ntl_mapres_gap_cuts must return, from the downloaded records: :443-489 with assess_accepted_anchor_contigs (:492-517)"""
    out = np.zeros(n, capi.GAP_CUT_DT)
    by_read = [[] for _ in range(n)]
    for m in rec["maps"]:
        by_read[int(m["read"])].append(m)
    stats = {"n_hits": set(), "accepted": set()}
    for g, maps in enumerate(by_read):
        stats["accepted"].add(len(maps))
        if len(maps) != 2:
            out[g]["status"] = capi.NTL_GAP_NOT_TWO
            continue
        maps.sort(key=lambda m: int(m["ctg"]))  # (in the order in which the read meets them: the target first in some)
        assert [int(m["ctg"]) for m in maps] == [2 * g, 2 * g + 1]
        stats["target_first"] = stats.get("target_first", 0) + (int(maps[0]["hit_off"]) > int(maps[1]["hit_off"]))
        sides, status = [], 0
        for m, minus, mixed_bit, pos_bit, source in ((maps[0], src_minus[g], capi.NTL_GAP_SRC_MIXED_STRANDS, capi.NTL_GAP_SRC_POSITIONS, True),
                                                     (maps[1], tgt_minus[g], capi.NTL_GAP_TGT_MIXED_STRANDS, capi.NTL_GAP_TGT_POSITIONS, False)):
            hits = [dict(ctg_pos=int(h["ctg_pos"]), read_pos=int(h["read_pos"]), ctg_strand=int(h["ctg_strand"]), read_strand=int(h["read_strand"]))
                    for h in rec["hits"][int(m["hit_off"]):int(m["hit_off"]) + int(m["n_hits"])]]
            stats["n_hits"].add(len(hits))
            ori, sign = find_orientation(hits), "-" if minus else "+"
            status |= (mixed_bit if ori is None else 0) | (0 if check_position_consistency(hits) else pos_bit)
            if source:
                terminal = hits[-1] if sign == ori else hits[0]
            else:
                terminal = hits[0] if sign == ori else hits[-1]
            sides.append((terminal["ctg_pos"], assign_read_cut(terminal["read_pos"], ori, sign, k), assign_ctg_cut(terminal["ctg_pos"], ori, sign, k),
                          ori == "+"))
        if status:
            out[g]["status"] = status
            continue
        out[g] = (0, *sides[0][:3], *sides[1][:3], int(sides[0][3]) | int(sides[1][3]) << 1)
    return out, stats


def check_random(dev):
    scaffolds, reads, src_minus, tgt_minus = random_gaps()
    n = len(reads)
    ctg_len = np.array([len(s) for s in scaffolds], np.uint32)
    read_len = np.array([len(s) for s in reads], np.uint32)
    with dev.batch(scaffolds) as sb, dev.batch(reads) as rb, dev.sketch(sb, K, W) as ssk, dev.sketch(rb, K, W) as rsk, \
            dev.map_grouped(ssk, ctg_len, 2 * np.arange(n + 1, dtype=np.uint32), rsk, read_len, np.arange(n + 1, dtype=np.uint32), k=K, z=100) as res:
        got = res.gap_cuts(src_minus, tgt_minus, K)  # on the pending result
        rec = res.download()
        again = res.gap_cuts(src_minus, tgt_minus, K)  # and on the completed one
    want, stats = restated(rec, n, src_minus, tgt_minus, K)
    # the coverage this test relies on
    valid = want[want["status"] == 0]
    assert {1, 2, 63, 64, 65} <= stats["n_hits"] and max(stats["n_hits"]) > 128, sorted(stats["n_hits"])
    assert 0 < stats["target_first"] < len(valid)
    assert {0, 1, 2} <= stats["accepted"] and int(rec["maps"]["read"][-2]) == n - 1, "the last gap has two mappings"
    assert len(valid) > n // 3 and {0, 3} <= set(valid["ori"].tolist())
    ok = want["status"] == 0  # the situations A-D (the contig's sign, the read-based orientation) on either side
    assert {(int(m), int(o) & 1) for m, o in zip(src_minus[ok], want["ori"][ok])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(int(m), int(o) >> 1) for m, o in zip(tgt_minus[ok], want["ori"][ok])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for bit in (capi.NTL_GAP_SRC_MIXED_STRANDS, capi.NTL_GAP_TGT_MIXED_STRANDS, capi.NTL_GAP_SRC_POSITIONS, capi.NTL_GAP_TGT_POSITIONS):
        assert (want["status"] & bit).any(), f"no gap with status bit {bit}"
    assert (want["status"] == capi.NTL_GAP_TGT_POSITIONS).any() and (want["status"] == capi.NTL_GAP_SRC_POSITIONS).any()
    for g in np.flatnonzero(got != want)[:5]:
        raise AssertionError(f"gap {g}: {got[g]}, the restated reference gives {want[g]}")
    assert (again == got).all()
    dev.sync()


# ---------------------------------------------------------------- c. errors

def check_errors(dev):
    def refused(res, n):
        with pytest.raises(capi.NtlError) as e:
            res.gap_cuts(np.zeros(n, np.uint8), np.zeros(n, np.uint8), K)
        assert e.value.code == capi.NTL_EINVAL and len(str(e.value)) > len("error -1: "), str(e.value)

    case = ic.array_case("a-7")
    with dev.sketch_from_arrays(case.coff, case.ch, case.cp, case.cs) as csk, dev.index(csk, case.ctg_len) as ix, \
            dev.sketch_from_arrays(*[case.reads[i] for i in (0, 2, 3, 4)]) as rsk, dev.map(ix, rsk, case.reads[1], k=gc.K) as res:
        refused(res, len(case.reads[1]))  # an ordinary result
    comp = gc.crafted("a")
    assert list(comp.cgo) != [2 * g for g in range(len(comp.cgo))]
    with dev.sketch_from_arrays(comp.coff, comp.ch, comp.cp, comp.cs) as csk, dev.sketch_from_arrays(comp.roff, comp.rh, comp.rp, comp.rs) as rsk, \
            dev.map_grouped(csk, comp.ctg_len, comp.cgo, rsk, comp.rlen, comp.rgo, k=gc.K) as res:
        refused(res, len(comp.rlen))  # groups of another shape
    scaffolds, reads, src_minus, tgt_minus = random_gaps()
    scaffolds, reads, n = scaffolds[:16], reads[:8], 8
    with dev.batch(scaffolds) as sb, dev.batch(reads) as rb, dev.sketch(sb, K, W) as ssk, dev.sketch(rb, K, W) as rsk:
        res = dev.map_grouped(ssk, np.array([len(s) for s in scaffolds], np.uint32), 2 * np.arange(n + 1, dtype=np.uint32), rsk,
                              np.array([len(s) for s in reads], np.uint32), np.arange(n + 1, dtype=np.uint32), k=K, z=100)
        refused(res, n - 1)
        refused(res, n + 1)
        got = res.gap_cuts(src_minus[:n], tgt_minus[:n], K)
        res.close()  # destroyed right after the call
        assert len(got) == n and (got["status"] == 0).any()
    dev.sync()


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    dev = simlib.device()
    yield dev
    dev.close()


def test_sim_golden(sim_dev, tmp_path):
    check_golden(sim_dev, tmp_path, False)


def test_sim_golden_stringent_in_batches(sim_dev, tmp_path):
    check_golden(sim_dev, tmp_path, True, batch_bases=150000)


def test_sim_random(sim_dev):
    check_random(sim_dev)


def test_sim_errors(sim_dev):
    check_errors(sim_dev)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    dev = capi.Device(0)
    yield dev
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stringent", [False, True])
def test_gpu_golden(gpu_dev, tmp_path, stringent):
    check_golden(gpu_dev, tmp_path, stringent)


@pytest.mark.gpu
@pytest.mark.parametrize("stringent", [False, True])
def test_gpu_golden_in_batches(gpu_dev, tmp_path, stringent):
    check_golden(gpu_dev, tmp_path, stringent, batch_bases=30000)


@pytest.mark.gpu
def test_gpu_random(gpu_dev):
    check_random(gpu_dev)


@pytest.mark.gpu
def test_gpu_errors(gpu_dev):
    check_errors(gpu_dev)
