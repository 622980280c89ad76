"""
The compiled host's wide-gate test circuit against Python's, without a GPU: host/bin/plonk_check --circuit-only builds the circuit of
zkhost::sample_circuit_wide and prints the SHA-256 of its tables before any device is touched; zkhip.plonk.sample_circuit_wide must
give the same bytes.  The transcript replay of the compiled host needs a proof record, and the compiled host has no prover without a
device: that half (one digest for one seed, the verdicts) is in tests/test_gpu_widegate.py.
"""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scalable-collaborative-zksnark_amd", "host")
PLONK_CHECK = os.path.join(HOST, "bin", "plonk_check")


@pytest.fixture(scope="module")
def plonk_check():
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/plonk_check"])

    def run(*args):
        return subprocess.run([PLONK_CHECK, *args], capture_output=True, text=True, timeout=120)

    return run


def _digest(c, selectors):
    h = hashlib.sha256()
    for k in tuple(selectors) + ("a", "b", "c", "public_inputs", "s", "sigma"):
        h.update(np.ascontiguousarray(c[k], dtype="<u8").tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("mu,seed", [(2, 3), (4, 7), (10, 7)])
def test_sample_circuit_is_the_same_in_both_hosts(plonk_check, mu, seed):
    from zkhip import plonk

    N = 1 << mu
    for flags, kw in (((), {}), (("--break-gate", str(N - 1)), {"break_gate": N - 1}), (("--break-wire", str(N - 2)), {"break_wire": N - 2})):
        r = plonk_check("--mu", str(mu), "--seed", str(seed), "--gate", "wide", "--circuit-only", *flags)
        m = re.fullmatch(r"circuit sha256 ([0-9a-f]{64})\n", r.stdout)
        assert r.returncode == 0 and m, (r.returncode, r.stdout, r.stderr)
        assert m.group(1) == _digest(plonk.sample_circuit_wide(mu, seed, **kw), plonk.WIDE_SELECTORS), flags
    r = plonk_check("--mu", str(mu), "--seed", str(seed), "--circuit-only")  # the basic kind through the same mode
    assert r.returncode == 0 and r.stdout == f"circuit sha256 {_digest(plonk.sample_circuit(mu, seed), ('q1', 'q2'))}\n"


def test_arguments_are_checked_before_any_device(plonk_check):
    for args in (("--mu", "4", "--gate"), ("--mu", "4", "--gate", "basic"), ("--mu", "4", "--gate", "wide", "--break-wire", "1"),
                 ("--mu", "4", "--gate", "wide", "--break-gate", "16"), ("--mu", "1", "--gate", "wide")):
        r = plonk_check(*args)
        assert r.returncode == 2 and not r.stdout, (args, r.returncode, r.stdout, r.stderr)
