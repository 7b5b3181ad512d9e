"""The stitch-paths stage (ntlink_amd/stitch_paths.py, Device.path_chains -> ntl_path_chains, csrc/path_kernels.h) -- under the SIMT
mock and on the GPU, the same checks.
  a. every golden case (tests/golden/gen_goldens_stitch.py: the reference's own ntlink_stitch_paths.py on crafted path files) through
     stitch_paths.stitch_paths(args, dev): the output file byte for byte; the four shipped .stitch.path files given back as they are
  b. Device.path_chains on crafted edge lists against the restatement of :221-365 in tests/path_cases.py: chains of 2, 3, 63, 64, 65
     and 1 025 vertices, 300 two-vertex chains, cycles of 2, 3 and 64 beside chains, chains that are their own twin, isolated
     vertices, a branch vertex with 2 and with 65 new in-edges, the transitive filter on a chain of 65 and on cycles
  c. 200 random symmetric graphs of at most 200 vertices, record for record
  d. the refusals of the C call"""
import argparse
import gzip
import json
import os

import numpy as np
import pytest

import path_cases as pc
from ntlink_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gen", "stitch_cases.json.gz")
SHIPPED = os.path.join(HERE, "golden", "ref", "expected_outputs")


# ---------------------------------------------------------------- a. the stage

def golden_cases():
    with gzip.open(GOLDEN, "rt") as fh:
        return json.load(fh)


def run_case(dev, case, tmp):
    from ntlink_amd import stitch_paths
    os.makedirs(tmp, exist_ok=True)
    for name, text in case["files"].items():
        with open(os.path.join(tmp, name), "w") as fh:
            fh.write(text)
    a = case["args"]
    args = argparse.Namespace(PATH=[os.path.join(tmp, p) for p in a["PATH"]], min_n=a["min_n"], max_n=a["max_n"], g=os.path.join(tmp, a["g"]),
                              a=a["a"], max_gap=a["max_gap"], o=os.path.join(tmp, "out.path"), p="out", transitive=a["transitive"],
                              conservative=a["conservative"])
    stitch_paths.stitch_paths(args, dev)
    with open(args.o) as fh:
        return fh.read()


def check_goldens(dev, tmp_path):
    cases = golden_cases()
    assert len(cases) >= 10
    assert {(c["args"]["conservative"], c["args"]["transitive"]) for c in cases.values()} == {(True, False), (False, False), (False, True)}
    for name, case in cases.items():
        got = run_case(dev, case, str(tmp_path / name))
        assert got == case["output"], f"case {name}: the stage wrote\n{got}the reference wrote\n{case['output']}"
    dev.sync()


def check_shipped(dev, tmp_path):
    """each shipped .stitch.path as the only path file, with a crafted .sterr, --conservative and scaf_num=None: the same bytes"""
    from ntlink_amd import stitch_paths
    names = sorted(f for f in os.listdir(SHIPPED) if f.endswith(".stitch.path"))
    assert len(names) == 4
    for name in names:
        with open(os.path.join(SHIPPED, name)) as fh:
            text = fh.read()
        path = str(tmp_path / name)
        with open(path, "w") as fh:
            fh.write(text)
        with open(path + ".sterr", "w") as fh:
            fh.write("n\tn:500\tL50\tmin\tN75\tN50\tN25\tE-size\tmax\tsum\tname\n")
            fh.write("30\t25\t5\t1000\t2000\t3000\t4000\t3500\t9000\t90000\tn=1 s=1000\n")
        dot = str(tmp_path / (name + ".dot"))
        with open(dot, "w") as fh:
            fh.write("digraph g {\ngraph [scaf_num=None]\n}\n")
        args = argparse.Namespace(PATH=[path], min_n=1, max_n=1, g=dot, a=0.3, max_gap=-1, o=path + ".out", p="out", transitive=False, conservative=True)
        stitch_paths.stitch_paths(args, dev)
        with open(args.o) as fh:
            assert fh.read() == text, name
    dev.sync()


# ---------------------------------------------------------------- b, c. the chains

def check_crafted(dev):
    for name in pc.crafted():
        pc.compare(dev, name)
    # what the cases are there for, on the restatement's own answers
    for n in (2, 3, 63, 64, 65, 1025):
        paths, *_ = pc.expected(f"chain-{n}")
        assert len(paths) == 1 and len(paths[0][0]) == n
    assert len(pc.expected("chains-300x2")[0]) == 300
    paths, _, _, no_source = pc.expected("cycles")
    assert no_source == 6 and [len(p[0]) for p in paths] == [3, 3, 3]  # every ring and its twin
    paths, *_ = pc.expected("self-twin")
    assert sorted(len(p[0]) for p in paths) == [2, 4, 6] and all(p[0][0] == p[0][-1] ^ 1 for p in paths if len(p[0]) > 2)
    assert pc.expected("isolated-only")[0] == []
    for fan in (2, 65):
        assert pc.expected(f"branch-{fan}-unique")[1] == 2 * (fan - 1) and max(len(p[0]) for p in pc.expected(f"branch-{fan}-unique")[0]) == 4
        assert pc.expected(f"branch-{fan}-tie")[1] == 2 * fan
        assert pc.expected(f"branch-{fan}-notnew")[1] == 2 * (fan - 1) and max(len(p[0]) for p in pc.expected(f"branch-{fan}-notnew")[0]) == 4
    paths, _, removed, _ = pc.expected("transitive-65")
    assert removed == 2 and [len(p[0]) for p in paths] == [64]  # the last new edge (63, 64) has target support alone; it goes with its twin
    paths, _, removed, _ = pc.expected("transitive-kinds")
    assert removed == 6 and sorted(len(p[0]) for p in paths) == [2, 2, 4, 4]
    paths, _, removed, no_source = pc.expected("transitive-cycle")
    assert removed == 2 and no_source == 2 and [len(p[0]) for p in paths] == [5]
    assert pc.expected("conservative")[1] == 0 and len(pc.expected("conservative")[0]) == 1
    dev.sync()


def check_random(dev):
    batches = pc.random_batches()
    assert len(batches) == 8 and all(g.n_vertices <= 25 * 200 for g, _ in batches)
    removed_lin = removed_trans = cycles = 0
    for i in range(len(batches)):
        _, a, b, c = pc.compare(dev, i)
        removed_lin, removed_trans, cycles = removed_lin + a, removed_trans + b, cycles + c
    assert removed_lin > 100 and removed_trans > 20 and cycles > 4
    dev.sync()


def check_errors(dev):
    g = pc.Graph()
    g.chain(pc.plus(g.contigs(3)))
    edges, links = g.arrays()

    def refused(n_vertices, ed, lk=links, mode=pc.STITCH):
        with pytest.raises(capi.NtlError) as e:
            dev.path_chains(n_vertices, ed, lk, mode)
        assert e.value.code == capi.NTL_EINVAL, str(e.value)
        return str(e.value)

    assert "twin" in refused(6, edges[:-1])
    bad = edges.copy()
    bad["d"][1] += 1
    assert "twin" in refused(6, bad)  # the twin is there, with another d
    assert "twice" in refused(6, np.concatenate([edges, edges[:2]]))
    assert "beyond n_vertices" in refused(4, edges)
    assert "beyond n_vertices" in refused(6, edges, np.array([(0, 6)], capi.PATH_LINK_DT), pc.TRANSITIVE)
    assert "odd" in refused(7, edges)
    assert "mode" in refused(6, edges, mode=3)
    fork = pc.Graph()
    a, b, c = pc.plus(fork.contigs(3))
    fork.edge(a, c)
    fork.edge(b, c)  # two in-edges that are not new: linearize leaves them
    assert "not linear" in refused(6, fork.arrays()[0])
    off, vertex, d, counts = np.zeros(4, np.uint32), np.zeros(6, np.uint32), np.zeros(6, np.int32), np.zeros(1, capi.PATH_COUNTS_DT)
    call = lambda ed, n_ed, lk, n_lk, o=off, v=vertex: dev.L.ntl_path_chains(dev.ptr, 6, ed, n_ed, lk, n_lk, pc.TRANSITIVE, o.ctypes.data if o is not None else None,
                                                                             v.ctypes.data if v is not None else None, d.ctypes.data, counts.ctypes.data)
    assert call(None, len(edges), None, 0) == capi.NTL_EINVAL  # NULL with a non-zero count
    assert call(edges.ctypes.data, len(edges), None, 1) == capi.NTL_EINVAL
    assert call(edges.ctypes.data, len(edges), None, 0, o=None) == capi.NTL_EINVAL
    assert call(edges.ctypes.data, len(edges), None, 0, v=None) == capi.NTL_EINVAL
    assert call(edges.ctypes.data, len(edges), None, 0) == 0 and int(counts["n_chains"][0]) == 1  # and the context still works
    assert len(dev.path_chains(0, edges[:0])[0]) == 1 and len(dev.path_chains(6, edges[:0])[1]) == 0
    dev.sync()


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    dev = simlib.device()
    yield dev
    dev.close()


def test_sim_goldens(sim_dev, tmp_path):
    check_goldens(sim_dev, tmp_path)


def test_sim_shipped(sim_dev, tmp_path):
    check_shipped(sim_dev, tmp_path)


def test_sim_crafted(sim_dev):
    check_crafted(sim_dev)


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
def test_gpu_goldens(gpu_dev, tmp_path):
    check_goldens(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_shipped(gpu_dev, tmp_path):
    check_shipped(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_crafted(gpu_dev):
    check_crafted(gpu_dev)


@pytest.mark.gpu
def test_gpu_random(gpu_dev):
    check_random(gpu_dev)


@pytest.mark.gpu
def test_gpu_errors(gpu_dev):
    check_errors(gpu_dev)
