"""From the chosen reads to the final cuts without the two temporary files (ntlink_amd.gapfill: get_gap_fill_reads, resident_scaffolds,
mask_ranges, gap_cuts_resident, map_long_reads_resident, print_masked_sequences) -- under the SIMT mock and on the GPU, the same checks.
The fixture tests/golden/gen/gapmask_cases.json.gz (tests/golden/gen_goldens_gapmask.py) holds unmasked scaffolds and reads, the pairs
with their chosen read and preset cuts, the two files the reference's own print_masked_sequences wrote for them and the end state its
map_long_reads left, --stringent off and on.
  a. print_masked_sequences writes the fixture's two files byte for byte; mask_ranges gives the ranges those files show
  b. gap_cuts_resident == gap_cuts over the fixture's files, record for record, in one batch and in batches of a few gaps
  c. map_long_reads_resident leaves the fixture's end state, both settings
  d. get_gap_fill_reads over two read files keeps the chosen reads only, and of a repeated id the later record
  e. 200 of test_gap_cuts.random_gaps()'s gaps embedded as scaffold ends and read pieces in longer records: the resident path gives
     the cut records gap_cut_sequences gives over the Python-masked records"""
import argparse
import functools
import gzip
import json
import os
import types

import numpy as np
import pytest

import test_gap_cuts as tgc
from ntlink_amd import capi, gapfill

HERE = os.path.dirname(os.path.abspath(__file__))
K, W = tgc.K, tgc.W
ACGT = np.frombuffer(b"ACGT", np.uint8)


@functools.lru_cache(maxsize=None)
def golden():
    with gzip.open(os.path.join(HERE, "golden", "gen", "gapmask_cases.json.gz"), "rt") as fh:
        doc = json.load(fh)
    assert len(doc["pairs"]) >= 11 and [s["stringent"] for s in doc["sets"]] == [False, True]
    return doc


def fresh(doc):
    """pairs and sequences as they stand before the masking step"""
    pairs = {}
    for source, target, chosen, sc, sr, tc, tr in doc["pairs"]:
        p = gapfill.PairInfo(100)
        p.chosen_read, p.source_ctg_cut, p.source_read_cut, p.target_ctg_cut, p.target_read_cut = chosen, sc, sr, tc, tr
        pairs[(source, target)] = p
    sequences = {name: types.SimpleNamespace(seq=seq, length=len(seq), five_prime_cut=0, three_prime_cut=len(seq)) for name, seq in doc["scaffolds"]}
    return pairs, sequences


def namespace(doc, prefix=None, stringent=False):
    return argparse.Namespace(o=prefix, k=doc["k"], w=doc["w"], z=doc["z"], x=doc["x"], sensitive=doc["sensitive"], stringent=stringent)


def write_files(doc, tmp_path):
    prefix = str(tmp_path / "g")
    for suffix, key in ((".scaffolds.masked_temp.fa", "scaffolds"), (".reads.masked_temp.fa", "reads")):
        with open(prefix + suffix, "w") as fh:
            fh.write(doc["files"][key])
    return prefix


def records_of(text):
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) % 2 == 1
    return [(lines[i][1:], lines[i + 1]) for i in range(0, len(lines) - 1, 2)]


# ---------------------------------------------------------------- a. the writer and the ranges (host code)

def test_print_masked_sequences_bytes(tmp_path):
    doc = golden()
    pairs, sequences = fresh(doc)
    prefix = str(tmp_path / "w")
    gapfill.print_masked_sequences(sequences, dict(doc["reads"]), pairs, namespace(doc, prefix))
    for suffix, key in ((".scaffolds.masked_temp.fa", "scaffolds"), (".reads.masked_temp.fa", "reads")):
        with open(prefix + suffix, "rb") as fh:
            assert fh.read() == doc["files"][key].encode(), key
    # from bytes and from plain sequences as well
    gapfill.print_masked_sequences({n: s.encode() for n, s in doc["scaffolds"]}, {i: s.encode() for i, s in doc["reads"]}, pairs, namespace(doc, prefix))
    with open(prefix + ".scaffolds.masked_temp.fa", "rb") as fh:
        assert fh.read() == doc["files"]["scaffolds"].encode()
    pairs[("x*", "sA+")] = pairs[("sA+", "sB+")]
    with pytest.raises(ValueError, match=r"\* must be \+ or -"):
        gapfill.print_masked_sequences(sequences, dict(doc["reads"]), pairs, namespace(doc, prefix))


def test_mask_ranges():
    doc = golden()
    pairs, _sequences = fresh(doc)
    scaffolds, reads = dict(doc["scaffolds"]), dict(doc["reads"])
    r = gapfill.mask_ranges(pairs, {n: len(s) for n, s in scaffolds.items()}, {i: len(s) for i, s in reads.items()})
    chosen = [(key, p) for key, p in pairs.items() if p.chosen_read is not None]
    n = len(chosen)
    assert r.keys == [key for key, _p in chosen] and n == len(pairs) - 1 and r.read_ids == [p.chosen_read for _key, p in chosen]
    assert r.src_minus.tolist() == [int(s[-1] == "-") for (s, _t), _p in chosen] and r.tgt_minus.tolist() == [int(t[-1] == "-") for (_s, t), _p in chosen]
    in_file = records_of(doc["files"]["scaffolds"])
    assert len(in_file) == 2 * n == len(r.scaffold_names) == len(r.scaffold_lo) == len(r.scaffold_hi)
    for i, (rid, line) in enumerate(in_file):
        seq, lo, hi = scaffolds[r.scaffold_names[i]], int(r.scaffold_lo[i]), int(r.scaffold_hi[i])
        assert rid == r.keys[i // 2][i % 2] + ("_target" if i % 2 else "_source")
        assert "N" * lo + seq[lo:hi] + "N" * (len(seq) - hi) == line, rid
    for g, (rid, line) in enumerate(records_of(doc["files"]["reads"])):
        seq, lo, hi = reads[r.read_ids[g]], int(r.read_lo[g]), int(r.read_hi[g])
        assert rid == f"{r.read_ids[g]}__{r.keys[g][0]}__{r.keys[g][1]}"
        assert "N" * lo + seq[lo:hi] + "N" * (len(seq) - hi) == line, rid
    assert (r.read_lo == r.read_hi).any() and (r.scaffold_lo == r.scaffold_hi).any()
    # refusals: the reference's ValueError, and cuts beyond a sequence
    lengths, rlengths = {n: len(s) for n, s in scaffolds.items()}, {i: len(s) for i, s in reads.items()}
    bad = dict(pairs)
    bad[("sA+", "sB")] = pairs[("sA+", "sB+")]
    with pytest.raises(ValueError, match=r"B must be \+ or -"):
        gapfill.mask_ranges(bad, dict(lengths, s=1), rlengths)
    for field, value in (("source_ctg_cut", lengths["sA"] + 1), ("target_ctg_cut", lengths["sB"] + 1), ("target_read_cut", rlengths["r_pp"] + 1)):
        pairs2, _ = fresh(doc)
        setattr(pairs2[("sA+", "sB+")], field, value)
        with pytest.raises(ValueError, match="outside"):
            gapfill.mask_ranges(pairs2, lengths, rlengths)


# ---------------------------------------------------------------- b. c. the resident path against the file path and the fixture

def residents(dev, doc):
    pairs, _ = fresh(doc)
    chosen = {p.chosen_read for p in pairs.values()} - {None}
    scaffolds = gapfill.resident_scaffolds(doc["scaffolds"], dev=dev)
    reads = gapfill.resident_scaffolds([(i, s) for i, s in doc["reads"] if i in chosen], dev=dev)
    return scaffolds, reads


def check_against_files(dev, tmp_path, batch_bases):
    doc = golden()
    prefix = write_files(doc, tmp_path)
    pairs, _ = fresh(doc)
    args = namespace(doc, prefix)
    want = gapfill.gap_cuts(prefix + ".scaffolds.masked_temp.fa", prefix + ".reads.masked_temp.fa", doc["k"], doc["w"], args, dev=dev)
    scaffolds, reads = residents(dev, doc)
    with scaffolds, reads:
        got = gapfill.gap_cuts_resident(pairs, scaffolds, reads, doc["k"], doc["w"], args, dev=dev, batch_bases=batch_bases)
    assert got.read_ids == want.read_ids and got.scaffold_ids == want.scaffold_ids
    assert got.src_minus.tolist() == want.src_minus.tolist() and got.tgt_minus.tolist() == want.tgt_minus.tolist()
    for g in np.flatnonzero(got.cuts != want.cuts)[:5]:
        raise AssertionError(f"gap {g} ({got.read_ids[g]}): {got.cuts[g]}, over the files {want.cuts[g]}")
    assert (want.cuts["status"] == 0).sum() >= 5 and (want.cuts["status"] != 0).sum() >= 3
    dev.sync()


def check_end_state(dev, stringent, batch_bases=gapfill.BATCH_BASES):
    doc = golden()
    exp = doc["sets"][int(stringent)]
    pairs, sequences = fresh(doc)
    scaffolds, reads = residents(dev, doc)
    with scaffolds, reads:
        gapfill.map_long_reads_resident(pairs, sequences, scaffolds, reads, namespace(doc, None, stringent), dev=dev, batch_bases=batch_bases)
    for g, (p, want, tag) in enumerate(zip(pairs.values(), exp["pairs"], doc["tags"])):
        got = [p.source_ctg_cut, p.source_read_cut, p.target_ctg_cut, p.target_read_cut, p.old_anchor_used]
        assert got == want, f"pair {g} ({tag}), stringent={stringent}: {got}, the reference leaves {want}"
    assert {name: [s.five_prime_cut, s.three_prime_cut] for name, s in sequences.items()} == exp["scaffolds"]
    # the fixture's own reach: new cuts and fallbacks, a scaffold cut at both ends
    used = [w[4] for w in doc["sets"][0]["pairs"]]
    assert any(used) and not all(used)
    assert 0 < exp["scaffolds"]["sG"][0] < exp["scaffolds"]["sG"][1] < len(dict(doc["scaffolds"])["sG"])
    dev.sync()


# ---------------------------------------------------------------- d. the reads collector

def check_gap_fill_reads(dev, tmp_path):
    doc = golden()
    pairs, _ = fresh(doc)
    reads = dict(doc["reads"])
    chosen = [i for i, _s in doc["reads"] if any(p.chosen_read == i for p in pairs.values())]
    assert len(chosen) == len(reads) and len({p.chosen_read for p in pairs.values()}) < len(pairs), "one read serves two pairs, one pair has none"
    fq, fa = str(tmp_path / "a.fq"), str(tmp_path / "b.fa")
    other = "ACGTTGCA" * 30
    later = reads["r_mm"][::-1]
    with open(fq, "w") as fh:
        for rid in ["stranger1"] + chosen[:5] + ["stranger2"]:
            seq = reads.get(rid, other)
            fh.write(f"@{rid} a comment\n{seq}\n+\n{'I' * len(seq)}\n")
    with open(fa, "w") as fh:
        for rid, seq in [(i, reads[i]) for i in chosen[5:]] + [("stranger3", other), ("r_mm", later)]:
            fh.write(f">{rid}\n{seq}\n")
    assert "r_mm" in chosen[:5]
    want = dict(reads, r_mm=later)
    with gapfill.get_gap_fill_reads([fq, fa], pairs, None, dev=dev, keep_ascii=True) as got:
        assert got.ids == chosen and got.lengths.tolist() == [len(want[i]) for i in chosen]
        assert got.number == {rid: i for i, rid in enumerate(chosen)} and got.batch.nseq == len(chosen)
        buf, off = got.batch.download_n()
        for i, rid in enumerate(chosen):
            assert buf[int(off[i]):int(off[i + 1])].tobytes() == want[rid].upper().encode(), rid
            assert got[rid] == want[rid].encode()
    with gapfill.get_gap_fill_reads([fq], pairs, None, dev=dev) as got:
        assert got.ids == chosen[:5]
        with pytest.raises(ValueError):
            got[chosen[0]]
    dev.sync()


# ---------------------------------------------------------------- e. random gaps, embedded in longer records

@functools.lru_cache(maxsize=None)
def embedded(n=200, seed=31):
    """test_gap_cuts.random_gaps()'s first n gaps as the ends of longer scaffolds and as pieces of longer reads ->
    (scaffold records, read records, pairs, Python-masked scaffold records, Python-masked read records)"""
    scaffolds, reads, src_minus, tgt_minus = tgc.random_gaps()
    rng = np.random.default_rng(seed)
    extra = lambda: ACGT[rng.integers(0, 4, int(rng.choice([0, 1, 15, 16, 17, int(rng.integers(18, 300))])))].tobytes()
    full_s, full_r, pairs, masked_s, masked_r = [], [], {}, [], []
    for g in range(n):
        nodes = []
        for side, seq, minus in ((0, scaffolds[2 * g], src_minus[g]), (1, scaffolds[2 * g + 1], tgt_minus[g])):
            name, more = f"{'st'[side]}{g}", extra()
            tail = bool(minus) != (side == 0)  # source +, target -: the kept end is the record's tail
            full_s.append((name, more + seq if tail else seq + more))
            cut = len(more) if tail else len(seq)
            node = name + "-+"[not minus]
            masked_s.append((node + ("_target" if side else "_source"), b"N" * len(more) + seq if tail else seq + b"N" * len(more)))
            nodes.append((node, cut))
        pre, post = extra(), extra()
        full_r.append((f"r{g}", pre + reads[g] + post))
        masked_r.append((f"r{g}__{nodes[0][0]}__{nodes[1][0]}", b"N" * len(pre) + reads[g] + b"N" * len(post)))
        p = gapfill.PairInfo(100)
        p.chosen_read, p.source_ctg_cut, p.target_ctg_cut = f"r{g}", nodes[0][1], nodes[1][1]
        p.source_read_cut, p.target_read_cut = (len(pre), len(pre) + len(reads[g]))[::(-1 if g & 1 else 1)]
        pairs[(nodes[0][0], nodes[1][0])] = p
    return full_s, full_r, pairs, masked_s, masked_r


def check_embedded(dev):
    full_s, full_r, pairs, masked_s, masked_r = embedded()
    args = argparse.Namespace(k=K, w=W, z=100, x=0.0, sensitive=False)
    want = gapfill.gap_cut_sequences(masked_s, masked_r, K, W, args, dev=dev)
    with gapfill.resident_scaffolds(full_s, dev=dev) as scaffolds, gapfill.resident_scaffolds(full_r, dev=dev) as reads:
        got = gapfill.gap_cuts_resident(pairs, scaffolds, reads, K, W, args, dev=dev)
        some = gapfill.gap_cuts_resident(pairs, scaffolds, reads, K, W, args, dev=dev, batch_bases=40000)
    assert got.read_ids == want.read_ids and got.scaffold_ids == want.scaffold_ids
    for g in np.flatnonzero(got.cuts != want.cuts)[:5]:
        raise AssertionError(f"gap {g}: {got.cuts[g]}, over the Python-masked records {want.cuts[g]}")
    assert (some.cuts == want.cuts).all()
    ok = want.cuts["status"] == 0
    assert ok.sum() > len(ok) // 3 and (~ok).sum() > 10 and {0, 3} <= set(want.cuts["ori"][ok].tolist())
    dev.sync()


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    dev = simlib.device()
    yield dev
    dev.close()


def test_sim_against_files(sim_dev, tmp_path):
    check_against_files(sim_dev, tmp_path, gapfill.BATCH_BASES)


def test_sim_against_files_in_batches(sim_dev, tmp_path):
    check_against_files(sim_dev, tmp_path, 12000)


def test_sim_end_state(sim_dev):
    check_end_state(sim_dev, False)


def test_sim_end_state_stringent_in_batches(sim_dev):
    check_end_state(sim_dev, True, batch_bases=12000)


def test_sim_gap_fill_reads(sim_dev, tmp_path):
    check_gap_fill_reads(sim_dev, tmp_path)


def test_sim_embedded(sim_dev):
    check_embedded(sim_dev)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    dev = capi.Device(0)
    yield dev
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("batch_bases", [gapfill.BATCH_BASES, 12000])
def test_gpu_against_files(gpu_dev, tmp_path, batch_bases):
    check_against_files(gpu_dev, tmp_path, batch_bases)


@pytest.mark.gpu
@pytest.mark.parametrize("stringent", [False, True])
def test_gpu_end_state(gpu_dev, stringent):
    check_end_state(gpu_dev, stringent)


@pytest.mark.gpu
def test_gpu_end_state_in_batches(gpu_dev):
    check_end_state(gpu_dev, False, batch_bases=12000)


@pytest.mark.gpu
def test_gpu_gap_fill_reads(gpu_dev, tmp_path):
    check_gap_fill_reads(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_embedded(gpu_dev):
    check_embedded(gpu_dev)
