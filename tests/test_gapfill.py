"""ntlink_amd.gapfill against the reference's own map_long_reads (tests/golden/gen/gapmap_cases.json.gz, made by
tests/golden/gen_goldens_gapmap.py): per gap the accepted contigs, their order and their hits -- under the SIMT mock and on the GPU."""
import argparse
import functools
import gzip
import json
import os

import pytest

from ntlink_amd import capi, gapfill

HERE = os.path.dirname(os.path.abspath(__file__))
SPECIAL = ["one_flank", "internal_repeat", "shared_flank_1", "shared_flank_2", "short_scaffold", "read_all_N", "scaffold_all_N", "equal_names"]


@functools.lru_cache(maxsize=None)
def golden():
    with gzip.open(os.path.join(HERE, "golden", "gen", "gapmap_cases.json.gz"), "rt") as fh:
        doc = json.load(fh)
    assert len(doc["reads"]) >= 60 and len(doc["scaffolds"]) == 2 * len(doc["reads"]) and all(t in doc["tags"] for t in SPECIAL)
    return doc


def test_default_name_of():
    assert [gapfill.default_name_of(s) for s in ("scaf12+_source", "-scaf_7-_target", "a_source_b+_target", "plain")] == \
        ["scaf12", "scaf_7", "a_source_b", "plain"]


def check_golden(dev, sensitive, batch_bases=gapfill.BATCH_BASES):
    doc = golden()
    one = next(s for s in doc["sets"] if bool(s["params"]["sensitive"]) == sensitive)
    p = one["params"]
    args = argparse.Namespace(k=p["k"], z=p["z"], x=p["x"], sensitive=p["sensitive"])
    gaps = list(gapfill.map_gap_sequences(doc["scaffolds"], doc["reads"], doc["k"], doc["w"], args, dev=dev, batch_bases=batch_bases))
    assert len(gaps) == len(one["gaps"])
    two = 0
    for g, (gap, exp, tag) in enumerate(zip(gaps, one["gaps"], doc["tags"])):
        assert gap.read.id == doc["reads"][g][0] and gap.read.readlen == len(doc["reads"][g][1]) and gap.read.num == g
        assert gap.source.id == doc["scaffolds"][2 * g][0] and gap.target.id == doc["scaffolds"][2 * g + 1][0]
        assert gap.target.readlen == len(doc["scaffolds"][2 * g + 1][1]) and gap.target.num == 2 * g + 1
        assert gap.order == exp["order"], f"gap {g} ({tag}): accepted contigs {gap.order}, the reference's {exp['order']}"
        assert list(gap.accepted) == exp["order"]
        for ctg in exp["order"]:
            run = gap.accepted[ctg]
            got = [[h.mx, h.ctg_pos, h.ctg_strand, h.read_pos, h.read_strand] for h in run.hits]
            assert run.contig == ctg and run.hit_count == len(got)
            assert got == exp["hits"][ctg], f"gap {g} ({tag}), contig {ctg}: the hits differ from the reference's"
        two += len(gap.order) == 2
    assert 2 * two >= len(gaps)
    dev.sync()


def check_minimizers_and_errors(dev):
    """with_minimizers=True: the records carry their sketch; a scaffold count other than twice the read count raises"""
    doc = golden()
    args = argparse.Namespace(k=doc["k"], z=1000, x=0.0, sensitive=False)
    first = doc["tags"].index("equal_names")
    gaps = list(gapfill.map_gap_sequences(doc["scaffolds"][2 * first:2 * first + 4], doc["reads"][first:first + 2], doc["k"], doc["w"], args,
                                          dev=dev, with_minimizers=True))
    exp = doc["sets"][0]["gaps"][first:first + 2]
    assert [g.order for g in gaps] == [e["order"] for e in exp]
    for gap in gaps:
        pos = [m.pos for m in gap.read.minimizers]
        assert pos == sorted(pos) and len(gap.source.minimizers) + len(gap.target.minimizers) > 0
        by_pos = {m.pos: str(m.out_hash) for m in gap.read.minimizers}
        assert all(by_pos[h.read_pos] == h.mx for run in gap.accepted.values() for h in run.hits)
    with pytest.raises(ValueError):
        list(gapfill.map_gap_sequences(doc["scaffolds"][:3], doc["reads"][:2], doc["k"], doc["w"], args, dev=dev))
    dev.sync()


def check_files(dev, tmp_path):
    """map_gap_reads over two FASTA files == map_gap_sequences; batches of a few gaps each"""
    doc = golden()
    n = 12
    args = argparse.Namespace(k=doc["k"], z=1000, x=0.0, sensitive=False)
    paths = []
    for nm, recs in (("scaffolds.fa", doc["scaffolds"][:2 * n]), ("reads.fa", doc["reads"][:n])):
        paths.append(str(tmp_path / nm))
        with open(paths[-1], "w") as fh:
            for rid, seq in recs:
                fh.write(f">{rid}\n{seq}\n")
    gaps = list(gapfill.map_gap_reads(paths[0], paths[1], doc["k"], doc["w"], args, dev=dev, batch_bases=40000))
    assert [g.order for g in gaps] == [e["order"] for e in doc["sets"][0]["gaps"][:n]]
    assert [g.read.id for g in gaps] == [r[0] for r in doc["reads"][:n]] and [g.read.num for g in gaps] == list(range(n))
    with open(paths[0], "a") as fh:
        fh.write(">extra_source\nACGT\n")
    with pytest.raises(ValueError):
        list(gapfill.map_gap_reads(paths[0], paths[1], doc["k"], doc["w"], args, dev=dev))
    dev.sync()


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    dev = simlib.device()
    yield dev
    dev.close()


@pytest.mark.parametrize("sensitive", [False, True])
def test_sim_golden(sim_dev, sensitive):
    check_golden(sim_dev, sensitive)


def test_sim_minimizers_and_errors(sim_dev):
    check_minimizers_and_errors(sim_dev)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    dev = capi.Device(0)
    yield dev
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sensitive", [False, True])
def test_gpu_golden(gpu_dev, sensitive):
    check_golden(gpu_dev, sensitive)


@pytest.mark.gpu
def test_gpu_golden_in_batches(gpu_dev):
    check_golden(gpu_dev, False, batch_bases=60000)


@pytest.mark.gpu
def test_gpu_minimizers_and_errors(gpu_dev):
    check_minimizers_and_errors(gpu_dev)


@pytest.mark.gpu
def test_gpu_files(gpu_dev, tmp_path):
    check_files(gpu_dev, tmp_path)
