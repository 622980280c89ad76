"""
The compiled host's host/bin/poseidon_check against tools/poseidon_merkle.py: without a device both print one circuit digest and one
host-rule root (--sample-only); on the device both print the same four lines for depth 1 and 2 at seed 7, and both report the refusal of a
path whose public root is wrong.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
CHECK = os.path.join(HOST, "bin", "poseidon_check")
TOOL = os.path.join(ROOT, "tools", "poseidon_merkle.py")


def both(*args):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/poseidon_check"])
    cpp = subprocess.run([CHECK, *args], capture_output=True, text=True, timeout=600)
    py = subprocess.run([sys.executable, TOOL, *args], capture_output=True, text=True, timeout=600)
    return cpp, py


@pytest.mark.parametrize("depth", [1, 2])
def test_sample_only_agrees_without_a_device(depth):
    cpp, py = both("--depth", str(depth), "--seed", "7", "--sample-only")
    assert cpp.returncode == 0 and py.returncode == 0, (cpp.stderr, py.stderr)
    lines = cpp.stdout.splitlines()
    assert lines == py.stdout.splitlines() and len(lines) == 2
    assert lines[0].startswith("circuit sha256 ") and lines[1].startswith("root ") and len(lines[1]) == 5 + 64


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2])
def test_four_lines_agree_on_the_device(depth):
    cpp, py = both("--depth", str(depth), "--seed", "7")
    assert cpp.returncode == 0 and py.returncode == 0, (cpp.stdout, cpp.stderr, py.stdout, py.stderr)
    lines = cpp.stdout.splitlines()
    assert lines == py.stdout.splitlines() and len(lines) == 4
    assert [ln.split()[0] for ln in lines] == ["circuit", "root", "proof", "verdict"] and lines[3] == "verdict accept"


@pytest.mark.gpu
def test_a_wrong_root_is_refused_in_both():
    cpp, py = both("--depth", "1", "--seed", "7", "--break", "root")
    assert cpp.returncode == 1 and py.returncode == 1, (cpp.stdout, cpp.stderr, py.stdout, py.stderr)
    assert cpp.stdout.splitlines() == py.stdout.splitlines()
    assert cpp.stdout.splitlines()[2].startswith("refused: zk_plonk_witness: 1 of 1536 slots differ from the value of their class")
