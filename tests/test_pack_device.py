"""The device-side ingest against a plain statement of the batch layout (tests/pack_cases.py) -- under the SIMT mock and on the GPU, the
same checks.  For every batch: nseq, bases, download_n() (text and offsets), the sketch at (k, w) = (3, 1) against the plain k-mer starts,
the sketches at (3, 1) and (4, 2) against the oracle's, and download(): the input back for a pure batch, NTL_EINVAL "pure-ACGT" otherwise.
  a. bit sweep: run starts, run ends and sequence boundaries at every bit of a 32-position group, 32 shifts
  b. no sequences, empty ones, all-N ones, one base; totals that end at 0, 1, 15, 16, 17, 31 modulo 32; every byte value
  c. block seams (8192 positions) and a scan over more than one tile
  d. offsets[0] = 5 and 16
  e. 100 random batches over five alphabets
  f. the letter-only cases through a FASTA file and the two packed constructors
  g. the purity flag of every constructor: ASCII, packed, packed-at, synthetic, masked; synth_slices refuses an impure source"""
import pytest

import pack_cases as pc
from ntlink_amd import capi


def check_sweep(dev):
    pc.check_cases(dev, pc.bit_sweep())


def check_edges(dev):
    pc.check_cases(dev, pc.degenerate() + pc.tails() + pc.every_byte())


def check_seams(dev):
    pc.check_cases(dev, pc.seams())


def check_random(dev):
    pc.check_cases(dev, pc.random_batches())


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    dev = simlib.device()
    yield dev
    dev.close()


def test_sim_sweep(sim_dev):
    check_sweep(sim_dev)


def test_sim_edges(sim_dev):
    check_edges(sim_dev)


def test_sim_seams(sim_dev):
    check_seams(sim_dev)


def test_sim_first_offset(sim_dev):
    pc.check_first_offset(sim_dev)


def test_sim_random(sim_dev):
    check_random(sim_dev)


def test_sim_packed_constructors(sim_dev, tmp_path, monkeypatch):
    from sim import simlib
    monkeypatch.setenv("NTLINK_AMD_LIB", simlib.build())  # the host parser of the same build
    pc.check_packed_constructors(sim_dev, tmp_path)


def test_sim_guards(sim_dev):
    pc.check_guards(sim_dev)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    dev = capi.Device(0)
    yield dev
    dev.close()


@pytest.mark.gpu
def test_gpu_sweep(gpu_dev):
    check_sweep(gpu_dev)


@pytest.mark.gpu
def test_gpu_edges(gpu_dev):
    check_edges(gpu_dev)


@pytest.mark.gpu
def test_gpu_seams(gpu_dev):
    check_seams(gpu_dev)


@pytest.mark.gpu
def test_gpu_first_offset(gpu_dev):
    pc.check_first_offset(gpu_dev)


@pytest.mark.gpu
def test_gpu_random(gpu_dev):
    check_random(gpu_dev)


@pytest.mark.gpu
def test_gpu_packed_constructors(gpu_dev, tmp_path):
    pc.check_packed_constructors(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_guards(gpu_dev):
    pc.check_guards(gpu_dev)
