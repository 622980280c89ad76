"""
The compiled host's gate ZeroCheck (host/examples/gate_check.cpp, zkhost/zerocheck.hpp): same proof record as the Python host
(one digest for one seed), accept / reject through the device pairing, and the refusal to run without a GPU.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
BIN = os.path.join(HOST, "bin", "gate_check")


def _build():
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/gate_check"])


def test_gate_check_builds_and_refuses_without_a_gpu():
    _build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([BIN], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "no CPU fallback" in r.stderr, (r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
def test_gate_check_accepts_with_the_python_hosts_digest(ctx):
    from zkhip import dist_primitive as dp
    from zkhip import zerocheck as zc

    _build()
    n, seed = 12, 7
    r = subprocess.run([BIN, "--n", str(n), "--seed", str(seed), "--digest"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "accept" in r.stdout, (r.returncode, r.stdout, r.stderr)
    got = re.search(r"proof sha256 ([0-9a-f]{64})", r.stdout).group(1)
    tabs, tau, chal, s = zc.satisfied_circuit(ctx, n, seed)
    proof = zc.gate_zerocheck_prove(ctx, dp.PolynomialCommitmentCub.new(ctx, s).mature(), tabs, tau, chal)
    assert zc.verify_rounds(proof, tau, chal)
    assert zc.proof_digest(proof) == got


@pytest.mark.gpu
def test_gate_check_rejects_a_broken_gate():
    _build()
    r = subprocess.run([BIN, "--n", "12", "--seed", "7", "--break-gate", "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "reject" in r.stdout, (r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
def test_gate_check_rejects_a_replaced_proof_point_through_the_device_pairing():
    """the field checks pass (the rounds and the opened values are the honest ones): the verdict is zk_pcs_verify_batch's"""
    _build()
    for table in ("0", "4"):
        r = subprocess.run([BIN, "--n", "12", "--seed", "7", "--break-opening", table], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "reject" in r.stdout and "final identity): ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    r = subprocess.run([BIN, "--n", "12", "--seed", "7", "--break-gate", "5"], capture_output=True, text=True, timeout=300)
    assert "final identity): failed" in r.stdout
