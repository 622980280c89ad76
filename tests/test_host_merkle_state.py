"""
The compiled host's host/bin/poseidon_check --update against tools/poseidon_merkle.py --update: without a device both print one circuit digest
and the host rules' old and new root (--sample-only); on the device both apply the writes to the tree they keep there, prove the transition
and print the same five lines, for one and two writes at depth 1 and 2, seed 7; a broken old leaf is refused by `witness` in both.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
CHECK = os.path.join(HOST, "bin", "poseidon_check")
TOOL = os.path.join(ROOT, "tools", "poseidon_merkle.py")
CASES = [(1, 1), (1, 2), (2, 1), (2, 2)]


def both(*args):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/poseidon_check"])
    cpp = subprocess.run([CHECK, *args], capture_output=True, text=True, timeout=600)
    py = subprocess.run([sys.executable, TOOL, *args], capture_output=True, text=True, timeout=600)
    return cpp, py


@pytest.mark.parametrize("depth,count", CASES)
def test_sample_only_agrees_without_a_device(depth, count):
    cpp, py = both("--depth", str(depth), "--seed", "7", "--update", str(count), "--sample-only")
    assert cpp.returncode == 0 and py.returncode == 0, (cpp.stderr, py.stderr)
    lines = cpp.stdout.splitlines()
    assert lines == py.stdout.splitlines() and len(lines) == 3
    assert lines[0].startswith("circuit sha256 ") and lines[1].startswith("old root ") and lines[2].startswith("new root ")
    assert len(lines[1]) == 9 + 64 and len(lines[2]) == 9 + 64 and lines[1][9:] != lines[2][9:]


def test_sample_only_is_the_model():
    """the printed roots are the independent model's: a tree of the seeded leaves, the seeded writes one after another"""
    import merkle_state_model as msm
    import poseidon_model as pm
    from zkhip.field import splitmix_fr

    depth, count, seed = 2, 2, 7
    n = 1 << depth
    _, py = both("--depth", str(depth), "--seed", str(seed), "--update", str(count), "--sample-only")
    tree = pm.merkle(msm.ints(splitmix_fr(n, seed)))
    writes = [((seed + 5 * k) % n, x) for k, x in enumerate(msm.ints(splitmix_fr(count, seed + 2)))]
    _, after = msm.chain(tree, n, writes)
    assert py.stdout.splitlines()[1:] == ["old root %064x" % tree[-1], "new root %064x" % after[-1][-1]]


def test_break_leaf_needs_update():
    cpp, py = both("--depth", "1", "--break", "leaf", "--sample-only")
    assert cpp.returncode == 2 and py.returncode == 2 and cpp.stdout == "" and py.stdout == ""


@pytest.mark.gpu
@pytest.mark.parametrize("depth,count", CASES)
def test_five_lines_agree_on_the_device(depth, count):
    cpp, py = both("--depth", str(depth), "--seed", "7", "--update", str(count))
    assert cpp.returncode == 0 and py.returncode == 0, (cpp.stdout, cpp.stderr, py.stdout, py.stderr)
    lines = cpp.stdout.splitlines()
    assert lines == py.stdout.splitlines() and len(lines) == 5
    assert [ln.split()[0] for ln in lines] == ["circuit", "old", "new", "proof", "verdict"] and lines[4] == "verdict accept"
    sample = subprocess.run([CHECK, "--depth", str(depth), "--seed", "7", "--update", str(count), "--sample-only"], capture_output=True, text=True, timeout=600)
    assert lines[:3] == sample.stdout.splitlines()


@pytest.mark.gpu
def test_a_broken_leaf_is_refused_in_both():
    cpp, py = both("--depth", "1", "--seed", "7", "--update", "1", "--break", "leaf")
    assert cpp.returncode == 1 and py.returncode == 1, (cpp.stdout, cpp.stderr, py.stdout, py.stderr)
    assert cpp.stdout.splitlines() == py.stdout.splitlines()
    assert cpp.stdout.splitlines()[3].startswith("refused: zk_plonk_witness: 1 of 3072 slots differ from the value of their class")
