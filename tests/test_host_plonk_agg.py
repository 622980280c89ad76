"""
Aggregated Plonk verification in the compiled host (host/zkhost/plonk.hpp: plonk_verify_many; host/bin/plonk_check --verify-many K
[--break-one J]) against the Python host (zkhip.plonk.verify_many).
Without a GPU: the binary builds with the new mode, its arguments are checked before any device is touched, it refuses to run without a
device, and --sample-only prints the digest it printed before (zkhip.plonk.circuit_digest).  With one (marked gpu): for the same
arguments both hosts print the same line -- the verdict list and the SHA-256 of the aggregate call's derived weights -- and the same
digest for every proof.  K proofs under the key of seed S: proof k is for the public inputs of seed S + k (wires from the device's
witness generator); with --lookup the proof of seed S is repeated.
"""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
BIN = os.path.join(HOST, "bin", "plonk_check")
MU, SEED = 4, 7


def _run(*args, gpu=False):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/plonk_check"])
    env = dict(os.environ) if gpu else dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120, env=env)


@pytest.mark.parametrize("args", [("--mu", "4", "--verify-many"), ("--mu", "4", "--verify-many", "0"), ("--mu", "4", "--verify-many", "257"),
                                  ("--mu", "4", "--break-one", "0"), ("--mu", "4", "--verify-many", "2", "--break-one", "2"),
                                  ("--mu", "4", "--verify-many", "2", "--bytes"), ("--mu", "4", "--verify-many", "2", "--break", "3"),
                                  ("--mu", "4", "--verify-many", "2", "--bad-input"), ("--mu", "4", "--verify-many", "2", "--sample-only")])
def test_usage_errors_of_verify_many(args):
    r = _run(*args)
    assert r.returncode == 2 and "usage: plonk_check" in r.stderr and "--verify-many K [--break-one J]" in r.stderr and not r.stdout, (args, r.returncode, r.stdout, r.stderr)


def test_verify_many_refuses_without_a_device():
    r = _run("--mu", "4", "--verify-many", "2")
    assert r.returncode == 2 and "no GPU visible" in r.stderr and not r.stdout, (r.returncode, r.stdout, r.stderr)


@pytest.mark.parametrize("kind,lookup", [(None, False), ("wide", False), (None, True)])
def test_sample_only_is_unaffected(kind, lookup):
    from zkhip import plonk

    c = plonk.sample_circuit_lookup(MU, SEED, gate=kind) if lookup else (plonk.sample_circuit_wide if kind else plonk.sample_circuit)(MU, SEED)
    r = _run("--mu", str(MU), "--seed", str(SEED), *_flags(kind, lookup), "--sample-only")
    assert r.returncode == 0 and r.stdout == f"circuit sha256 {plonk.circuit_digest(c)}\n", (r.returncode, r.stdout, r.stderr)


def _flags(kind, lookup):
    return (("--gate", "wide") if kind else ()) + (("--lookup",) if lookup else ())


def _python_lines(ctx, kind, lookup, K, J):
    """what plonk_check --verify-many K [--break-one J] prints, from the Python host"""
    import zerocheck_model as zm
    from zkhip import Ctx, plonk
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr

    sample = (lambda seed: plonk.sample_circuit_lookup(MU, seed, gate=kind)) if lookup else (lambda seed: (plonk.sample_circuit_wide if kind else plonk.sample_circuit)(MU, seed))
    c = sample(SEED)
    pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
    pk, vk = plonk.preprocess(ctx, pcs, c, pr.powers_of_g2(zm.ints(c["s"])))
    items = [(c["public_inputs"], plonk.prove(ctx, pk, c["a"], c["b"], c["c"], c["public_inputs"], **({"idx": c["idx"]} if lookup else {})))]
    plan = None if lookup else plonk.witness_plan(ctx, c)
    for k in range(1, K):
        if lookup:
            items.append(items[0])
            continue
        pi = sample(SEED + k)["public_inputs"]
        a, b, cc = plonk.witness(ctx, pk, plan, pi)
        items.append((pi, plonk.prove(ctx, pk, a, b, cc, pi)))
    if J is not None:
        opening = np.array(items[J][1]["batch"]["opening"], copy=True)
        opening[0] = opening[-1]
        items[J] = (items[J][0], dict(items[J][1], batch=dict(items[J][1]["batch"], opening=opening)))
    lines = [f"proof {k} sha256 {plonk.proof_digest(p)}" for k, (_, p) in enumerate(items)]
    rho = Ctx.pcs_agg_weights(*dp.agg_arrays(plonk.agg_openings(vk, items)[1]))
    verdicts = plonk.verify_many(ctx, vk, items)
    lines.append("verify-many K=%d verdicts %s weights sha256 %s" % (K, ",".join("1" if v else "0" for v in verdicts),
                                                                      hashlib.sha256(np.ascontiguousarray(rho, dtype="<u8").tobytes()).hexdigest()))
    return lines, verdicts


@pytest.mark.gpu
@pytest.mark.parametrize("kind,lookup,K,J", [(None, False, 3, None), (None, False, 3, 1), ("wide", False, 2, 0), (None, True, 2, None), (None, True, 2, 1),
                                             (None, False, 1, None)])
def test_both_hosts_print_one_verdict_and_weights_line(ctx, kind, lookup, K, J):
    want, verdicts = _python_lines(ctx, kind, lookup, K, J)
    # the repeated lookup proof: the broken copy alone is rejected, its twin (the same record, unbroken) is not
    assert verdicts == [k != J for k in range(K)]
    r = _run("--mu", str(MU), "--seed", str(SEED), *_flags(kind, lookup), "--verify-many", str(K), *(("--break-one", str(J)) if J is not None else ()), gpu=True)
    assert r.returncode == (0 if J is None else 1), (r.returncode, r.stdout, r.stderr)
    got = r.stdout.splitlines()
    assert got[:-1] == want, (got, want)
    assert re.fullmatch(r"plonk_check mu=4 N=16 l=4 seed=7.*: (accept|reject)", got[-1]) and got[-1].endswith("reject" if J is not None else "accept")
