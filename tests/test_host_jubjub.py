"""
The compiled host's Jubjub side (host/zkhost/jubjub.hpp through host/bin/poseidon_check) against the Python host (tools/poseidon_merkle.py):
without a GPU, --sample-only gives one circuit digest and one signature digest for the Schnorr circuit and for the signed transfer (honest and
forged), for two seeds -- so the builders agree row for row and signing gives the same bytes; on the device, both hosts print the same
circuit digest, signature, (roots,) proof digest and verdict, and the forged transfer is refused by both with one message.
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


@pytest.mark.parametrize("args,heads", [
    (("--schnorr", "--seed", "7"), ["circuit", "signature"]),
    (("--schnorr", "--seed", "12"), ["circuit", "signature"]),
    (("--depth", "2", "--seed", "7", "--signed-transfer", "--bits", "8"), ["circuit", "signature", "roots"]),
    (("--depth", "1", "--seed", "12", "--signed-transfer", "--bits", "16", "--amount", "9"), ["circuit", "signature", "roots"]),
    (("--depth", "2", "--seed", "7", "--signed-transfer", "--bits", "8", "--forge"), ["circuit", "signature", "roots"]),
])
def test_sample_only_digests_agree(args, heads):
    cpp, py = both(*args, "--sample-only")
    assert cpp.returncode == 0 and py.returncode == 0, (cpp.stdout, cpp.stderr, py.stdout, py.stderr)
    lines = cpp.stdout.splitlines()
    assert lines == py.stdout.splitlines() and [ln.split()[0] for ln in lines] == heads


def test_the_python_digests_are_the_modules():
    """the tool prints what zkhip.jubjub builds and signs: the digests above are those of schnorr_circuit() and sign_host"""
    import hashlib

    from zkhip import jubjub as jj
    from zkhip.circuit import circuit_digest

    cpp = subprocess.run([CHECK, "--schnorr", "--seed", "7", "--sample-only"], capture_output=True, text=True, timeout=600)
    assert cpp.stdout.splitlines() == ["circuit sha256 " + circuit_digest(jj.schnorr_circuit()[0]),
                                       "signature sha256 " + hashlib.sha256(jj.signature_bytes(jj.sign_host(8, 1007))).hexdigest()]


def test_the_compiled_serial_rule_runs():
    out = subprocess.run([CHECK, "--time-schnorr", "8"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("host schnorr verify n=8 ms ") and "0 refused" in out.stdout


@pytest.mark.gpu
def test_schnorr_four_lines_agree_on_the_device():
    cpp, py = both("--schnorr", "--seed", "7")
    assert cpp.returncode == 0 and py.returncode == 0, (cpp.stdout, cpp.stderr, py.stdout, py.stderr)
    lines = cpp.stdout.splitlines()
    assert lines == py.stdout.splitlines()
    assert [ln.split()[0] for ln in lines] == ["circuit", "signature", "proof", "verdict"] and lines[3] == "verdict accept"


@pytest.mark.gpu
def test_signed_transfer_five_lines_agree_on_the_device():
    cpp, py = both("--depth", "2", "--seed", "7", "--signed-transfer", "--bits", "8")
    assert cpp.returncode == 0 and py.returncode == 0, (cpp.stdout, cpp.stderr, py.stdout, py.stderr)
    lines = cpp.stdout.splitlines()
    assert lines == py.stdout.splitlines()
    assert [ln.split()[0] for ln in lines] == ["circuit", "signature", "roots", "proof", "verdict"] and lines[4] == "verdict accept"


@pytest.mark.gpu
def test_a_forged_transfer_is_refused_in_both():
    cpp, py = both("--depth", "2", "--seed", "7", "--signed-transfer", "--bits", "8", "--forge")
    assert cpp.returncode == 1 and py.returncode == 1, (cpp.stdout, cpp.stderr, py.stdout, py.stderr)
    assert cpp.stdout.splitlines() == py.stdout.splitlines()
    assert cpp.stdout.splitlines()[3].startswith("refused: zk_plonk_witness: ")
