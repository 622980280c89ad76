"""
Verifying-key bytes in the compiled host (host/zkhost/vk_io.hpp, host/bin/plonk_check) against the Python host (zkhip/vk_io.py).
Without a GPU: the binary builds, the arguments of the new modes are checked before any device is touched, the vk-layout vectors
(--vk-vectors: a synthetic key for both gate kinds with and without a lookup, read back by the serial rules, and the refusal of a key
plus a point of order 13) equal the Python host's bytes, and the compiled host's G2 rule (--g2check-time) gives the Python rule's points
bit for bit.  With one (marked gpu): for one seed both hosts write the same vk bytes; each host's file verifier accepts the other's three
files and refuses them, naming the key, with --vk-torsion.
"""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import g1check_model as g1m
import g2check_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
BIN = os.path.join(HOST, "bin", "plonk_check")
TOOL = os.path.join(ROOT, "tools", "plonk_verify.py")
MU, SEED = 4, 7
KINDS = [(None, False), (None, True), ("wide", False), ("wide", True)]


def _run(*args, gpu=False):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/plonk_check"])
    env = dict(os.environ) if gpu else dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120, env=env)


@pytest.mark.parametrize("args", [("--mu", "4", "--vk-torsion", "1"), ("--mu", "4", "--dump-vk", "x"), ("--mu", "4", "--dump-public", "x"),
                                  ("--mu", "4", "--bytes", "--vk-torsion"), ("--mu", "4", "--vk-vectors"), ("--vk-vectors", "--reps", "2"),
                                  ("--g2check-time", "0"), ("--mu", "4", "--g2check-time", "3"), ("--verify-files", "a", "b"),
                                  ("--mu", "4", "--verify-files", "a", "b", "c"), ("--host-checks",)])
def test_usage_errors_of_the_new_modes(args):
    r = _run(*args)
    assert r.returncode == 2 and not r.stdout, (args, r.returncode, r.stdout, r.stderr)


def test_the_vk_layout_vectors_equal_the_python_host_s():
    from zkhip import plonk, vk_io

    r = _run("--vk-vectors")
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert len(lines) == 4
    for line, (kind, lookup) in zip(lines, KINDS):
        k = vk_io.commitment_count(kind, lookup)
        vk = {"mu": MU, "l": 2, "pcs": None, "commitments": np.stack([g1m.words(g1m.mul(g1m.G, 3 + j)) for j in range(k)]),
              "g2": np.stack([gm.words(gm.mul(gm.G2, 5 + 7 * j)) for j in range(MU + 2)]), **({"gate": kind} if kind else {}), **({"lookup": True} if lookup else {})}
        data = plonk.vk_to_bytes(vk)
        want = (f"vk vectors gate={kind or 'basic'} lookup={int(lookup)} bytes {len(data)} sha256 {hashlib.sha256(data).hexdigest()} round_trip 1 "
                "torsion: G2 key 3: not in the subgroup")
        assert line == want


def test_the_compiled_host_rule_gives_the_python_rule_s_points():
    from zkhip import pairing as pr
    from zkhip import serialize as ser

    r = _run("--g2check-time", "7", "--reps", "1")
    m = re.fullmatch(r"g2check host points 7 ms [0-9.]+ all_ok 1 points_sha256 ([0-9a-f]{64})\n", r.stdout)
    assert r.returncode == 0 and m, (r.returncode, r.stdout, r.stderr)
    P, encs = None, []
    for _ in range(7):
        P = pr.g2_add(P, pr.G2_GEN)
        encs.append(ser.g2_serialize_compressed(P))
    pts, st = ser.g2_decompress_check_host(b"".join(encs))
    assert not st.any() and hashlib.sha256(np.ascontiguousarray(pts, dtype="<u8").tobytes()).hexdigest() == m.group(1)


def test_the_torsion_point_of_the_compiled_host_has_order_13():
    src = open(os.path.join(HOST, "examples", "plonk_check.cpp")).read()
    enc = bytes.fromhex(re.search(r'kOrder13\[\] = "([0-9a-f]{192})"', src).group(1))
    st, P = gm.decompress_check(enc)
    assert st == gm.NOT_IN_G2 and P is not None and gm.mul(P, 13) is None


_FILES = {}


def _python_files(ctx, kind, lookup):
    """the Python host's three byte strings for its own proof of the sample circuit (the circuit plonk_check proves for the same seed)"""
    if (kind, lookup) not in _FILES:
        import zerocheck_model as zm
        from zkhip import dist_primitive as dp
        from zkhip import pairing as pr
        from zkhip import plonk, vk_io

        c = plonk.sample_circuit_lookup(MU, SEED, gate=kind) if lookup else (plonk.sample_circuit_wide if kind else plonk.sample_circuit)(MU, SEED)
        pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
        pk, vk = plonk.preprocess(ctx, pcs, c, pr.powers_of_g2(zm.ints(c["s"])))
        proof = plonk.prove(ctx, pk, c["a"], c["b"], c["c"], c["public_inputs"], **({"idx": c["idx"]} if lookup else {}))
        _FILES[(kind, lookup)] = (plonk.vk_to_bytes(vk), plonk.proof_to_bytes(proof), vk_io.public_to_bytes(c["public_inputs"]))
    return _FILES[(kind, lookup)]


def _flags(kind, lookup):
    return (("--gate", "wide") if kind else ()) + (("--lookup",) if lookup else ())


@pytest.mark.gpu
@pytest.mark.parametrize("kind,lookup", KINDS)
def test_both_hosts_write_one_key_and_accept_each_other_s_files(ctx, tmp_path, kind, lookup):
    vkb, pfb, pib = _python_files(ctx, kind, lookup)
    paths = [str(tmp_path / n) for n in ("vk.bin", "proof.bin", "public.bin")]
    r = _run("--mu", str(MU), "--seed", str(SEED), *_flags(kind, lookup), "--bytes", "--dump-vk", paths[0], "--dump-proof", paths[1], "--dump-public", paths[2], gpu=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    m = re.search(r"^vk sha256 ([0-9a-f]{64}) \((\d+) bytes\)$", r.stdout, re.M)
    assert m and m.group(1) == hashlib.sha256(vkb).hexdigest() and int(m.group(2)) == len(vkb), r.stdout
    assert [open(p, "rb").read() for p in paths] == [vkb, pfb, pib]
    # the compiled host's files through the Python verifier (a fresh process), the same files through the compiled one
    want = "".join(f"{n}_sha256 {hashlib.sha256(b).hexdigest()} bytes {len(b)}\n" for n, b in zip(("vk", "proof", "public"), (vkb, pfb, pib))) + "verdict accepted\n"
    py = subprocess.run([sys.executable, TOOL, "--vk", paths[0], "--proof", paths[1], "--public", paths[2]], capture_output=True, text=True, timeout=120)
    assert py.returncode == 0 and py.stdout == want, (py.returncode, py.stdout, py.stderr)
    cc = _run("--verify-files", *paths, gpu=True)
    assert cc.returncode == 0 and cc.stdout == want, (cc.returncode, cc.stdout, cc.stderr)
    if kind is None:
        hc = _run("--verify-files", *paths, "--host-checks", gpu=True)
        assert hc.returncode == 0 and hc.stdout == want
    # other public inputs: rejected
    open(paths[2], "wb").write(bytes([pib[0] ^ 1]) + pib[1:])
    cc = _run("--verify-files", *paths, gpu=True)
    assert cc.returncode == 1 and cc.stdout.endswith("verdict rejected\n"), (cc.returncode, cc.stdout)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,lookup", [(None, False), ("wide", True)])
def test_vk_torsion_is_refused_by_both_hosts_naming_the_key(ctx, tmp_path, kind, lookup):
    from zkhip import vk_io

    vkb, pfb, pib = _python_files(ctx, kind, lookup)
    K = 2 if kind else MU + 1
    r = _run("--mu", str(MU), "--seed", str(SEED), *_flags(kind, lookup), "--bytes", "--vk-torsion", str(K), gpu=True)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    assert f"refused: G2 key {K}: not in the subgroup\n" in r.stdout and r.stdout.rstrip().endswith(": reject"), r.stdout
    # the same key in files: the Python host's key plus the model's point of order 13, through both file verifiers
    at = 26 + 48 * vk_io.commitment_count(kind, lookup) + 96 * K
    P = gm.add(gm.decompress_check(vkb[at:at + 96])[1], dict(gm.points(1))["order13"])
    paths = [str(tmp_path / n) for n in ("vk.bin", "proof.bin", "public.bin")]
    for p, b in zip(paths, (vkb[:at] + gm.compress(P) + vkb[at + 96:], pfb, pib)):
        open(p, "wb").write(b)
    line = f"verdict refused: G2 key {K}: not in the subgroup\n"
    cc = _run("--verify-files", *paths, gpu=True)
    assert cc.returncode == 2 and cc.stdout.endswith(line), (cc.returncode, cc.stdout, cc.stderr)
    py = subprocess.run([sys.executable, TOOL, "--vk", paths[0], "--proof", paths[1], "--public", paths[2], "--aggregate"], capture_output=True, text=True, timeout=120)
    assert py.returncode == 2 and py.stdout.endswith(line), (py.returncode, py.stdout, py.stderr)
    r = _run("--mu", str(MU), "--bytes", "--vk-torsion", str(MU + 2), gpu=True)
    assert r.returncode == 2 and "--vk-torsion names one of" in r.stderr
