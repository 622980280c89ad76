"""
The compiled host's lookup sample without a device: `lookup_check --sample-only` prints the digest of the table, the column and the
indices, which has to be the Python sampler's for the same seed.
"""
import os
import re
import subprocess

import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scalable-collaborative-zksnark_amd", "host")
LOOKUP_CHECK = os.path.join(HOST, "bin", "lookup_check")


def _sample_only(*args):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/lookup_check"])
    r = subprocess.run([LOOKUP_CHECK, *args, "--sample-only"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    return re.search(r"sample sha256 ([0-9a-f]{64})", r.stdout).group(1)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sample_digests_agree(seed):
    from zkhip import lookup as lk

    assert _sample_only("--n", "7", "--seed", str(seed)) == lk.sample_digest(*lk.sample_lookup(7, seed))
    assert _sample_only("--n", "5", "--seed", str(seed), "--distinct", "9") == lk.sample_digest(*lk.sample_lookup(5, seed, 9))


def test_arguments_are_checked_before_any_device_is_touched():
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/lookup_check"])
    for args in (["--n", "0"], ["--n", "4", "--break", "5"], ["--n", "4", "--break", "1", "--outside"], ["--n", "3", "--distinct", "9"], []):
        r = subprocess.run([LOOKUP_CHECK, *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (args, r.stdout, r.stderr)
