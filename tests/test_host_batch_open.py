"""
The compiled host's batch opening (host/examples/batch_open_check.cpp, zkhost/batch_open.hpp): the same proof record as the Python
host (one digest for one seed) and the same verdicts on the corrupted runs, through the device pairing.
"""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
BIN = os.path.join(HOST, "bin", "batch_open_check")
pytestmark = pytest.mark.gpu
N_VARS, SEED, TABLES, CLAIMS = 10, 7, 4, 9


def _run(*args, n=N_VARS, seed=SEED):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/batch_open_check"])
    return subprocess.run([BIN, "--n", str(n), "--seed", str(seed), "--tables", str(TABLES), "--claims", str(CLAIMS), *args], capture_output=True, text=True, timeout=300)


def _python_host(ctx, n=N_VARS, seed=SEED):
    from zkhip import batch_open as bo
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip.field import fr_from_mont

    N = 1 << n
    tables, pts, alpha, rho, s = bo.random_instance(ctx, n, TABLES, CLAIMS, seed)
    pcs = dp.PolynomialCommitmentCub.new(ctx, s).mature()
    comms = np.stack([dp.commit(ctx, pcs, t, N) for t in tables])
    claims = bo.evaluate_claims(ctx, tables, N, pts)
    proof = bo.batch_open_prove(ctx, pcs, tables, N, claims, alpha, rho)
    vk = dp.pcs_vk(ctx, pr.powers_of_g2([fr_from_mont(x) for x in s]))
    return bo, vk, comms, claims, proof, alpha, rho


@pytest.mark.parametrize("n,seed", [(10, 7), (6, 3), (13, 11)])
def test_both_hosts_print_the_same_digest_and_accept(ctx, n, seed):
    r = _run("--digest", n=n, seed=seed)
    assert r.returncode == 0 and "accept" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "check 1 (round chain from S): ok" in r.stdout and re.search(r"check 2\+3 \([^)]*\): ok", r.stdout), r.stdout
    got = re.search(r"proof sha256 ([0-9a-f]{64})", r.stdout).group(1)
    bo, vk, comms, claims, proof, alpha, rho = _python_host(ctx, n, seed)
    assert bo.proof_digest(proof) == got
    assert bo.batch_open_verify(ctx, vk, comms, claims, proof, alpha, rho) is True


def test_both_hosts_reject_a_corrupted_claimed_value_at_the_round_chain(ctx):
    from zkhip.field import fr_from_mont, fr_mont

    bo, vk, comms, claims, proof, alpha, rho = _python_host(ctx)
    for k in (0, 4, CLAIMS - 1):
        r = _run("--break-value", str(k))
        assert r.returncode == 1 and "reject" in r.stdout, (r.returncode, r.stdout, r.stderr)
        assert "check 1 (round chain from S): failed" in r.stdout, r.stdout
        bad = list(claims)
        bad[k] = (claims[k][0], claims[k][1], fr_mont(fr_from_mont(claims[k][2]) + 1))
        assert bo.failed_checks(TABLES, bad, proof, alpha, rho) == [1]
        assert bo.batch_open_verify(ctx, vk, comms, bad, proof, alpha, rho) is False


def test_both_hosts_reject_a_replaced_proof_point_through_the_device_pairing(ctx):
    """the field checks pass (the rounds and the claimed values are the honest ones): the verdict is zk_pcs_verify_batch's"""
    import pyoracle as po
    from helpers import jac_norm_to_affine, pt_ints

    r = _run("--break-opening")
    assert r.returncode == 1 and "reject" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "check 1 (round chain from S): ok" in r.stdout and re.search(r"check 2\+3 \([^)]*\): failed", r.stdout), r.stdout
    bo, vk, comms, claims, proof, alpha, rho = _python_host(ctx)
    k = N_VARS // 2
    other = po.g1_add(pt_ints(jac_norm_to_affine(proof["opening"][k])), po.G1_GEN)  # the same replacement: the point + g1
    bad = {"rounds": proof["rounds"], "opening": proof["opening"].copy()}
    bad["opening"][k] = np.concatenate([np.array(po.fq_to_mont_limbs(other[0]) + po.fq_to_mont_limbs(other[1]), dtype=np.uint64), proof["opening"][k][12:]])
    assert bo.failed_checks(TABLES, claims, bad, alpha, rho) == []
    assert bo.batch_open_verify(ctx, vk, comms, claims, bad, alpha, rho) is False
