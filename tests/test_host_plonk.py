"""
The compiled host's one-circuit proof (host/examples/plonk_check.cpp, zkhost/plonk.hpp) without a GPU: it builds, and argument errors
exit non-zero before any device is touched.  The proofs themselves are compared in tests/test_gpu_plonk.py.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
BIN = os.path.join(HOST, "bin", "plonk_check")


def _run(*args):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/plonk_check"])
    # no device is visible to the child: an argument error must be reported without asking for one
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120, env=env)


def test_plonk_check_builds():
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/plonk_check"])
    assert os.access(BIN, os.X_OK)


@pytest.mark.parametrize("args", [(), ("--mu",), ("--mu", "x"), ("--mu", "-3"), ("--seed", "7"), ("--mu", "10", "--frobnicate"), ("--mu", "10", "--seed"),
                                  ("--mu", "10", "--break-gate", "1", "--break-wire", "9"), ("--mu", "10", "--break-gate", "1", "--bad-input")])
def test_usage_errors(args):
    r = _run(*args)
    assert r.returncode == 2 and "usage: plonk_check" in r.stderr and not r.stdout, (args, r.returncode, r.stdout, r.stderr)


@pytest.mark.parametrize("args,word", [(("--mu", "1"), "--mu must be in"), (("--mu", "25"), "--mu must be in"), (("--mu", "4", "--break-gate", "16"), "--break-gate"),
                                       (("--mu", "4", "--break-wire", "16"), "--break-wire"), (("--mu", "4", "--break-wire", "3"), "--break-wire")])
def test_range_errors(args, word):
    r = _run(*args)
    assert r.returncode == 2 and word in r.stderr and "no GPU" not in r.stderr and not r.stdout, (args, r.returncode, r.stdout, r.stderr)
