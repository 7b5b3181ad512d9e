"""bin/ntlink_stitch_paths.py on a real MI355X, in a child process: the reference Makefile's two argument lines (ntLink:235-239) on a
golden case of tests/golden/gen_goldens_stitch.py, `-v`, and an unreadable `-g`."""
import os
import subprocess
import sys

import pytest

from test_stitch_paths import golden_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "ntlink_stitch_paths.py")


def _stage(tmp_path, case):
    for name, text in case["files"].items():
        (tmp_path / name).write_text(text)


def _run(tmp_path, *argv):
    return subprocess.run([sys.executable, TOOL, *argv], cwd=tmp_path, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("name,flags", [("stitch-max_gap-9", []), ("conservative", ["--conservative"])])
def test_makefile_lines(tmp_path, name, flags):
    case = golden_cases()[name]
    _stage(tmp_path, case)
    a = case["args"]
    got = _run(tmp_path, "--min_n", "1", "--max_n", "5", "-p", "out", "-g", a["g"], *flags, *a["PATH"], "-o", "s.stitch.path", "--max_gap", str(a["max_gap"]))
    assert got.returncode == 0, got.stderr
    assert (tmp_path / "s.stitch.path").read_text() == case["output"]
    out = got.stdout
    assert out.startswith("Running ntLink stitch paths stage...\n\n") and "Optimal n = 2 at N50 = 3000.0" in out
    assert "\nTotal number of components in graph: " in out
    if flags:
        assert "Printing paths for optimal N50, no stitching...\n" in out and "Reading" not in out
    else:
        assert "Reading s.n1.path\n" in out and "Reading s.n5.path\ns.n5.path does not exist, skipping.\n" in out and "Reading s.n2.path" not in out


def test_version_and_unreadable_graph(tmp_path):
    got = _run(tmp_path, "-v")
    assert got.returncode == 0 and "ntLink v1.3.11" in got.stdout
    case = golden_cases()["stitch"]
    _stage(tmp_path, case)
    (tmp_path / "s.stitch.path").write_text("stale\n")
    got = _run(tmp_path, "--min_n", "1", "--max_n", "5", "-g", "missing.dot", *case["args"]["PATH"], "-o", "s.stitch.path")
    assert got.returncode == 1 and "ERROR" in got.stderr and "missing.dot" in got.stderr
    assert not (tmp_path / "s.stitch.path").exists()
