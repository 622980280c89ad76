"""
The compiled host's wiring PermCheck (host/examples/wiring_check.cpp, zkhost/wiring.hpp): same proof record as the Python host
(one digest for one seed), accept / reject through the device pairing, and the refusal to run without a GPU.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
BIN = os.path.join(HOST, "bin", "wiring_check")


def _build():
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/wiring_check"])


def _run(*args):
    return subprocess.run([BIN, "--n", "10", "--seed", "7", *args], capture_output=True, text=True, timeout=300)


def test_wiring_check_builds_and_refuses_without_a_gpu():
    _build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([BIN], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "no CPU fallback" in r.stderr, (r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
def test_wiring_check_accepts_with_the_python_hosts_digest(ctx):
    from zkhip import dist_primitive as dp
    from zkhip import wiring as wr

    _build()
    mu, seed = 10, 7
    r = _run("--digest")
    assert r.returncode == 0 and "accept" in r.stdout, (r.returncode, r.stdout, r.stderr)
    for k in (1, 2, 3, 4):
        assert re.search(r"check %d \([^)]*\): ok" % k, r.stdout), r.stdout
    got = re.search(r"proof sha256 ([0-9a-f]{64})", r.stdout).group(1)
    w, sid, ssigma, alpha, beta, gamma, tau, chal, s = wr.permuted_circuit(ctx, mu, seed)
    proof = wr.wiring_prove(ctx, dp.PolynomialCommitmentCub.new(ctx, s).mature(), w, sid, ssigma, 1 << mu, alpha, beta, gamma, tau, chal)
    assert wr.verify_rounds(proof, alpha, beta, gamma, tau, chal)
    assert wr.proof_digest(proof) == got


@pytest.mark.gpu
def test_wiring_check_rejects_a_broken_wire_at_the_product_check():
    _build()
    r = _run("--break-wire", "5")
    assert r.returncode == 1 and "reject" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "check 3 (grand product = 1): failed" in r.stdout
    # the sumcheck of a consistent tree still closes, and the openings are honest
    for k in (1, 2, 4):
        assert re.search(r"check %d \([^)]*\): ok" % k, r.stdout), r.stdout


@pytest.mark.gpu
def test_wiring_check_rejects_a_replaced_proof_point_through_the_device_pairing():
    """the field checks pass (the rounds and the opened values are the honest ones): the verdict is zk_pcs_verify_batch's"""
    _build()
    for opening in ("1", "5", "7"):  # sid at r; the tree at (r,0) and at (1,..,1,0)
        r = _run("--break-opening", opening)
        assert r.returncode == 1 and "reject" in r.stdout, (r.returncode, r.stdout, r.stderr)
        for k in (1, 2, 3):
            assert re.search(r"check %d \([^)]*\): ok" % k, r.stdout), r.stdout
        assert re.search(r"check 4 \([^)]*\): failed", r.stdout), r.stdout
