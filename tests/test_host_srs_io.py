"""
Parameter-set bytes in the compiled host (host/zkhost/srs_io.hpp, host/bin/plonk_check --dump-srs / --srs) against the Python host
(zkhip/srs_io.py, tools/plonk_srs.py).  Without a GPU: the binary builds and the arguments of the new modes are checked before any
device is touched.  With one (marked gpu): for one seed both hosts write the same file; each host loads the other's file; plonk_check
--srs prints the proof digest it prints without the flag; both refuse a tampered file with the same message.
"""
import hashlib
import os
import re
import subprocess
import sys

import pytest

import g1check_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
BIN = os.path.join(HOST, "bin", "plonk_check")
TOOL = os.path.join(ROOT, "tools", "plonk_srs.py")
MU, SEED = 4, 7
N_VARS = MU + 1


def _run(*args, gpu=False):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/plonk_check"])
    env = dict(os.environ) if gpu else dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120, env=env)


def _tool(*args):
    return subprocess.run([sys.executable, TOOL, *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args", [("--mu", "4", "--dump-srs"), ("--mu", "4", "--srs"), ("--mu", "4", "--dump-srs", "a", "--srs", "b"),
                                  ("--mu", "4", "--circuit-only", "--srs", "a"), ("--mu", "4", "--verify-many", "2", "--dump-srs", "a"),
                                  ("--srs", "a")])
def test_usage_errors_of_the_new_modes(args):
    r = _run(*args)
    assert r.returncode == 2 and not r.stdout, (args, r.returncode, r.stdout, r.stderr)


_FILE = {}


def _python_file(ctx):
    """the Python host's file of the parameter set of the sample circuit's trapdoor (the circuit plonk_check proves for the same seed)"""
    if not _FILE:
        import zerocheck_model as zm
        from zkhip import dist_primitive as dp
        from zkhip import pairing as pr
        from zkhip import plonk

        c = plonk.sample_circuit(MU, SEED)
        pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
        _FILE["data"] = plonk.srs_to_bytes(ctx, pcs, pr.powers_of_g2(zm.ints(c["s"])))
    return _FILE["data"]


def _head(data):
    return f"srs_sha256 {hashlib.sha256(data).hexdigest()} bytes {len(data)}\n"


@pytest.mark.gpu
def test_both_hosts_write_one_file_and_load_each_other_s(ctx, tmp_path):
    data = _python_file(ctx)
    assert len(data) == 26 + 48 * 2**N_VARS + 96 * (N_VARS + 1)
    cc_path, py_path = str(tmp_path / "cc.srs"), str(tmp_path / "py.srs")
    plain = _run("--mu", str(MU), "--seed", str(SEED), gpu=True)
    assert plain.returncode == 0, (plain.returncode, plain.stdout, plain.stderr)
    r = _run("--mu", str(MU), "--seed", str(SEED), "--dump-srs", cc_path, gpu=True)
    assert r.returncode == 0 and r.stdout == _head(data) + plain.stdout, (r.returncode, r.stdout, r.stderr)
    assert open(cc_path, "rb").read() == data  # one file, hence one SHA-256, for one seed in both hosts
    # the compiled host's file through the Python loader (a fresh process)
    py = _tool("--check", cc_path)
    assert py.returncode == 0 and py.stdout.startswith(_head(data) + "verdict accepted"), (py.returncode, py.stdout, py.stderr)
    # the Python host's file through the compiled loader: the proof made on it has the digest of the proof made on the trapdoor's set
    open(py_path, "wb").write(data)
    cc = _run("--mu", str(MU), "--seed", str(SEED), "--srs", py_path, gpu=True)
    assert cc.returncode == 0 and cc.stdout == _head(data) + plain.stdout, (cc.returncode, cc.stdout, cc.stderr)
    assert re.search(r"^proof sha256 [0-9a-f]{64}$", plain.stdout, re.M) and plain.stdout.rstrip().endswith(": accept")
    # and through the bytes path, whose vk carries the loaded keys
    b0, b1 = _run("--mu", str(MU), "--seed", str(SEED), "--bytes", gpu=True), _run("--mu", str(MU), "--seed", str(SEED), "--bytes", "--srs", py_path, gpu=True)
    assert b0.returncode == 0 and b1.returncode == 0 and b1.stdout == _head(data) + b0.stdout, (b1.stdout, b1.stderr)


@pytest.mark.gpu
def test_one_file_serves_a_smaller_circuit_in_the_compiled_host(ctx, tmp_path):
    # the file of the mu = 5 circuit's trapdoor cut down to 5 variables is the set of its last five coordinates: not the mu = 4 circuit's
    # own set, so the digest differs from the plain run, but the proof made on it verifies against the loaded keys
    path = str(tmp_path / "big.srs")
    r = _run("--mu", str(MU + 1), "--seed", str(SEED), "--dump-srs", path, gpu=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    cc = _run("--mu", str(MU), "--seed", str(SEED), "--srs", path, gpu=True)
    assert cc.returncode == 0 and cc.stdout.rstrip().endswith(": accept"), (cc.returncode, cc.stdout, cc.stderr)
    small = _run("--mu", str(MU + 2), "--seed", str(SEED), "--srs", path, gpu=True)
    assert small.returncode == 2 and "more variables than the parameter set has" in small.stdout, (small.returncode, small.stdout, small.stderr)


@pytest.mark.gpu
def test_a_tampered_file_is_refused_by_both_hosts_with_one_message(ctx, tmp_path):
    from zkhip import pairing as pr
    from zkhip import serialize as ser

    data = _python_file(ctx)
    N = 1 << N_VARS

    def point_at(i):
        return gm.decompress_check(data[26 + 48 * i:26 + 48 * i + 48])[1]

    def with_point(i, P):
        return data[:26 + 48 * i] + gm.compress(P) + data[26 + 48 * i + 48:]

    key_at = 26 + 48 * N + 96 * 2
    cases = [
        (with_point(3, gm.add(point_at(3), (0, 2))), "G1 point 3: not in the subgroup"),
        (with_point(5, None), "G1 point 5: the point at infinity"),
        (data[:key_at] + ser.g2_serialize_compressed(pr.g2_mul(pr.G2_GEN, 4242)) + data[key_at + 96:], f"level {N_VARS - 1} does not match G2 key 2"),
        (data[:key_at] + ser.g2_serialize_compressed(None) + data[key_at + 96:], "G2 key 2: the point at infinity"),
        (with_point(N // 2 + 2, gm.neg(point_at(2))), f"level {N_VARS - 1}: 1 of {N // 2} sums are the point at infinity; the first is sum 2"),
        (data[:-1], f"{len(data) - 1} bytes, the header's parameter set has {len(data)}"),
    ]
    for k, (bad, msg) in enumerate(cases):
        path = str(tmp_path / f"bad{k}.srs")
        open(path, "wb").write(bad)
        want = _head(bad) + f"verdict refused: {msg}\n"
        cc = _run("--mu", str(MU), "--seed", str(SEED), "--srs", path, gpu=True)
        assert cc.returncode == 2 and cc.stdout == want, (k, cc.returncode, cc.stdout, cc.stderr)
        py = _tool("--check", path)
        assert py.returncode == 2 and py.stdout == want, (k, py.returncode, py.stdout, py.stderr)
    # a top-level point replaced by another member: both hosts name the same level
    path = str(tmp_path / "member.srs")
    open(path, "wb").write(with_point(N - 1, gm.mul(gm.G, 31337)))
    cc, py = _run("--mu", str(MU), "--seed", str(SEED), "--srs", path, gpu=True), _tool("--check", path)
    assert cc.returncode == 2 and py.returncode == 2 and cc.stdout == py.stdout and re.search(r"verdict refused: level \d does not match G2 key \d\n$", cc.stdout)
