"""
Proof bytes in the compiled host (host/zkhost/proof_io.hpp, host/bin/plonk_check --bytes) against the Python host (zkhip/proof_io.py).
Without a GPU: the binary builds, the arguments of the new modes are checked before any device is touched, and the compiled host's G1
rule (g1_decompress_check_host, serial big integers; --g1check-time) gives the Python rule's points bit for bit.  With one (marked gpu,
the compiled host has no prover without a device): for one seed both hosts print the same SHA-256 of the bytes, for both gate kinds
with and without --lookup; --dump-proof writes those bytes; --torsion K is refused naming point K.
"""
import hashlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
BIN = os.path.join(HOST, "bin", "plonk_check")
MU, SEED = 4, 7


def _run(*args, gpu=False):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/plonk_check"])
    env = dict(os.environ) if gpu else dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120, env=env)


@pytest.mark.parametrize("args", [("--mu", "4", "--torsion", "3"), ("--mu", "4", "--dump-proof", "x"), ("--mu", "4", "--bytes", "--torsion"),
                                  ("--mu", "4", "--bytes", "--break", "2"), ("--mu", "4", "--g1check-time", "3"), ("--g1check-time", "0"),
                                  ("--g1check-time", "3", "--reps", "0")])
def test_usage_errors_of_the_new_modes(args):
    r = _run(*args)
    assert r.returncode == 2 and "usage: plonk_check" in r.stderr and not r.stdout, (args, r.returncode, r.stdout, r.stderr)


def test_the_compiled_host_rule_gives_the_python_rule_s_points():
    import numpy as np

    from zkhip import pairing as pr
    from zkhip import serialize as ser

    r = _run("--g1check-time", "9", "--reps", "1")
    m = re.fullmatch(r"g1check host points 9 ms [0-9.]+ all_ok 1 points_sha256 ([0-9a-f]{64})\n", r.stdout)
    assert r.returncode == 0 and m, (r.returncode, r.stdout, r.stderr)
    P, encs = None, []
    for _ in range(9):
        P = pr.g1_add(P, pr.G1_GEN)
        encs.append(ser.g1_serialize_compressed(P))
    pts, st = ser.g1_decompress_check_host(b"".join(encs))
    assert not st.any() and hashlib.sha256(np.ascontiguousarray(pts, dtype="<u8").tobytes()).hexdigest() == m.group(1)


_BYTES = {}


def _python_bytes(ctx, kind, lookup):
    """the Python host's encoding of its own proof of the sample circuit (the circuit plonk_check proves for the same seed)"""
    if (kind, lookup) not in _BYTES:
        import zerocheck_model as zm
        from zkhip import dist_primitive as dp
        from zkhip import pairing as pr
        from zkhip import plonk

        c = plonk.sample_circuit_lookup(MU, SEED, gate=kind) if lookup else (plonk.sample_circuit_wide if kind else plonk.sample_circuit)(MU, SEED)
        pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
        pk, vk = plonk.preprocess(ctx, pcs, c, pr.powers_of_g2(zm.ints(c["s"])))
        proof = plonk.prove(ctx, pk, c["a"], c["b"], c["c"], c["public_inputs"], **({"idx": c["idx"]} if lookup else {}))
        _BYTES[(kind, lookup)] = plonk.proof_to_bytes(proof)
    return _BYTES[(kind, lookup)]


def _flags(kind, lookup):
    return (("--gate", "wide") if kind else ()) + (("--lookup",) if lookup else ())


KINDS = [(None, False), (None, True), ("wide", False), ("wide", True)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,lookup", KINDS)
def test_both_hosts_print_one_digest_of_the_bytes(ctx, tmp_path, kind, lookup):
    data = _python_bytes(ctx, kind, lookup)
    dump = str(tmp_path / "proof.bin")
    r = _run("--mu", str(MU), "--seed", str(SEED), *_flags(kind, lookup), "--bytes", "--dump-proof", dump, gpu=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    m = re.search(r"^bytes sha256 ([0-9a-f]{64}) \((\d+) bytes\)$", r.stdout, re.M)
    assert m and m.group(1) == hashlib.sha256(data).hexdigest() and int(m.group(2)) == len(data), r.stdout
    assert r.stdout.rstrip().endswith(": accept") and "refused" not in r.stdout
    assert open(dump, "rb").read() == data


@pytest.mark.gpu
@pytest.mark.parametrize("kind,lookup", [(None, False), ("wide", True)])
def test_torsion_is_refused_naming_the_point(ctx, kind, lookup):
    from zkhip import proof_io

    parts = proof_io.point_parts(kind, lookup, MU)
    names = sorted(set(p for p, _ in parts))
    for j, name in enumerate(names):  # one point of every part
        slots = [s for s, (p, _) in enumerate(parts) if p == name]
        K = slots[j % len(slots)]
        r = _run("--mu", str(MU), "--seed", str(SEED), *_flags(kind, lookup), "--bytes", "--torsion", str(K), gpu=True)
        assert r.returncode == 1, (K, r.returncode, r.stdout, r.stderr)
        assert f"refused: {proof_io.describe(*parts[K], 3)}\n" in r.stdout and r.stdout.rstrip().endswith(": reject"), (K, r.stdout)
    r = _run("--mu", str(MU), "--bytes", "--torsion", str(len(parts)), gpu=True)
    assert r.returncode == 2 and "--torsion names one of" in r.stderr
