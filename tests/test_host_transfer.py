"""
The compiled host's host/bin/poseidon_check --transfer against tools/poseidon_merkle.py --transfer on the device: the same four lines --
circuit digest, roots, proof digest, verdict -- for (depth, bits) = (1, 8) and (2, 16), and the same refusal for an amount of 0.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
CHECK = os.path.join(HOST, "bin", "poseidon_check")
TOOL = os.path.join(ROOT, "tools", "poseidon_merkle.py")

pytestmark = pytest.mark.gpu


def both(*args):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/poseidon_check"])
    cpp = subprocess.run([CHECK, *args], capture_output=True, text=True, timeout=600)
    py = subprocess.run([sys.executable, TOOL, *args], capture_output=True, text=True, timeout=600)
    return cpp, py


@pytest.mark.parametrize("depth,bits", [(1, 8), (2, 16)])
def test_four_lines_agree_on_the_device(depth, bits):
    cpp, py = both("--depth", str(depth), "--seed", "7", "--transfer", "--bits", str(bits))
    assert cpp.returncode == 0 and py.returncode == 0, (cpp.stdout, cpp.stderr, py.stdout, py.stderr)
    lines = cpp.stdout.splitlines()
    assert lines == py.stdout.splitlines() and len(lines) == 4
    assert [ln.split()[0] for ln in lines] == ["circuit", "roots", "proof", "verdict"] and lines[3] == "verdict accept"
    sample = subprocess.run([CHECK, "--depth", str(depth), "--seed", "7", "--transfer", "--bits", str(bits), "--sample-only"], capture_output=True, text=True, timeout=600)
    assert lines[:2] == sample.stdout.splitlines()


def test_an_amount_of_zero_is_refused_in_both():
    cpp, py = both("--depth", "1", "--seed", "7", "--transfer", "--bits", "8", "--amount", "0")
    assert cpp.returncode == 1 and py.returncode == 1, (cpp.stdout, cpp.stderr, py.stdout, py.stderr)
    assert cpp.stdout.splitlines() == py.stdout.splitlines()
    assert cpp.stdout.splitlines()[2].startswith("refused: zk_plonk_witness: 1 of 2048 rows do not satisfy the gate")
