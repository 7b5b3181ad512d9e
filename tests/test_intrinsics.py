"""The instruction wrappers of dev_intrin.h, one by one: the product's gfx950 bodies (ntlink_amd/csrc/dev_intrin.h, on the GPU) and
the SIMT mock's portable bodies (tests/sim/include/dev_intrin.h, on CPU threads) run the same probe kernels (tests/probe) over the same
operand tables and are compared, exactly, with the definitions restated in tests/intrin_cases.py: product == definition == mock.
The whole CPU suite runs the product's kernels over the mock's bodies, so a test that is green under the mock says something about the
GPU only as far as this file holds.  A wrapper that gets no probe fails test_every_wrapper_is_probed."""
import os
import re

import pytest

import intrin_cases as ic
from probe import probelib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = {"product": os.path.join(ROOT, "ntlink_amd", "csrc", "dev_intrin.h"), "mock": os.path.join(ROOT, "tests", "sim", "include", "dev_intrin.h")}
FUNCTION = re.compile(r"(?m)^(?:template\s*<[^>]*>\s*)?(?:__device__\s+__forceinline__|inline)\s[^;{(]*?\b(ntl_\w+)\s*\(")
MACRO = re.compile(r"(?m)^\s*#\s*define\s+(NTL_\w+)")
TYPEDEF = re.compile(r"(?m)^typedef\s[^;]*?\b(ntl_\w+)\s*;")


def defined_names(path):
    with open(path) as fh:
        text = fh.read()
    return set(FUNCTION.findall(text)) | set(MACRO.findall(text)) | set(TYPEDEF.findall(text))


def test_every_wrapper_is_probed():
    product, mock = defined_names(HEADERS["product"]), defined_names(HEADERS["mock"])
    assert len(product) >= 35
    assert product == mock, f"only the product's: {sorted(product - mock)}, only the mock's: {sorted(mock - product)}"
    assert not set(ic.PROBED) & set(ic.EXEMPT)
    missing = product - set(ic.PROBED) - set(ic.EXEMPT)
    assert not missing, f"no probe for {sorted(missing)}: add an operation to tests/probe/intrin_probe.hip and a table to tests/intrin_cases.py"
    stale = (set(ic.PROBED) | set(ic.EXEMPT)) - product
    assert not stale, f"{sorted(stale)} are no longer defined"
    assert set(ic.PROBED.values()) <= set(ic.CHECKS) and all(ic.EXEMPT.values())
    assert set(ic.CHECKS) - set(ic.PROBED.values()) == {"block_excl_scan"}  # dev_common.h's, built on ntl_wave_incl_scan


def test_mul_add_table_tells_fused_from_two_roundings():
    """on the reference alone: at least 20 triples of the table round differently when fused"""
    assert ic.mul_add_cases()[3] >= 20


CHECK_NAMES = sorted(ic.CHECKS)


@pytest.fixture(scope="module")
def sim_probe():
    return probelib.probe("sim")


@pytest.fixture(scope="module")
def gpu_probe():
    return probelib.probe("gpu")


@pytest.mark.parametrize("name", CHECK_NAMES)
def test_sim(sim_probe, name):
    ic.CHECKS[name](sim_probe)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CHECK_NAMES)
def test_gpu(gpu_probe, name):
    ic.CHECKS[name](gpu_probe)
