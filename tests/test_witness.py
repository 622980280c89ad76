"""
Witness generation without a GPU: the model of the rules (witness_model.py) reproduces the wires of all four samplers bit for bit, its
plan has the properties the hand-built circuits are made for, and the library, the binding and the Rust FFI carry the new symbols.
(zk_witness_plan_create takes a ctx, which needs a device: the plan properties of the LIBRARY are asserted in test_gpu_witness.py on the
same circuits and against the same model figures.)
"""
import ctypes
import os

import numpy as np
import pytest

import witness_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("zk_witness_plan_create", "zk_witness_plan_free", "zk_witness_plan_info", "zk_plonk_witness", "zk_plonk_witness_check")
KINDS = ("basic", "wide", "basic-lookup", "wide-lookup")


def sample(kind: str, mu: int, seed: int, **kw) -> dict:
    from zkhip import plonk

    gate = "wide" if kind.startswith("wide") else None
    if kind.endswith("lookup"):
        return plonk.sample_circuit_lookup(mu, seed, gate=gate, **kw)
    return (plonk.sample_circuit_wide if gate else plonk.sample_circuit)(mu, seed, **kw)


def model_plan(c: dict) -> dict:
    return wm.plan(c["sigma"], 1 << c["mu"], wm.computing_rows(c))


def free_of(c: dict):
    return wm.free_of_lookup(c) if "lookup" in c else None


@pytest.mark.parametrize("seed", [3, 7])
@pytest.mark.parametrize("mu", [3, 4, 6])
@pytest.mark.parametrize("kind", KINDS)
def test_model_reproduces_the_samplers(kind, mu, seed):
    c = sample(kind, mu, seed)
    p = model_plan(c)
    a, b, cc = wm.generate(c, p, c["public_inputs"], free_of(c))
    for name, got in (("a", a), ("b", b), ("c", cc)):
        assert (wm.limbs(got) == c[name]).all(), name
    assert wm.check(c, p, a, b, cc, c["public_inputs"]) == {"bad_rows": 0, "first_bad_row": None, "bad_copies": 0, "first_bad_copy": None}


@pytest.mark.parametrize("kind", ["basic", "wide"])
def test_model_check_reports_the_samplers_breaks(kind):
    mu = 5
    K = (1 << mu) - 1  # the last row: nothing copies its c, so the break stays in one place
    good = sample(kind, mu, 3)
    p = model_plan(good)
    c = sample(kind, mu, 3, break_gate=K)
    assert wm.check(c, p, wm.ints(c["a"]), wm.ints(c["b"]), wm.ints(c["c"]), c["public_inputs"]) == {"bad_rows": 1, "first_bad_row": K, "bad_copies": 0, "first_bad_copy": None}
    c = sample(kind, mu, 3, break_wire=K)
    assert wm.check(c, p, wm.ints(c["a"]), wm.ints(c["b"]), wm.ints(c["c"]), c["public_inputs"]) == {"bad_rows": 0, "first_bad_row": None, "bad_copies": 1, "first_bad_copy": K}


def test_new_symbols_exist():
    import zkhip
    from zkhip import _lib, plonk

    lib = ctypes.CDLL(zkhip.LIB_PATH)
    bound = {s[0] for s in _lib.SYMBOLS}
    rust = open(os.path.join(ROOT, "rust", "zkhip_sys.rs")).read()
    header = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in bound and f"pub fn {s}(" in rust and f"{s}(" in header, s
    for f in ("witness_plan", "witness", "check_witness"):
        assert callable(getattr(plonk, f)), f
    for f in ("witness_plan", "plonk_witness", "plonk_witness_check"):
        assert callable(getattr(zkhip.Ctx, f)), f


def test_chain_plan():
    """N - l + 1 levels (the deepest is level N - l), every one of at most 256 rows: one single-workgroup run"""
    mu, l = 10, 4
    N = 1 << mu
    p = model_plan(wm.chain(mu, l))
    assert [len(r) for r in p["levels"]] == [l] + [1] * (N - l)
    assert p["level"][N - 1] == N - l
    assert wm.info(p) == {"levels": N - l + 1, "max_level_rows": l, "launches": 1}


def test_flat_plan():
    """one level of N - l rows above the input rows: a launch of its own, after the run that holds the input rows"""
    mu, l = 10, 4
    N = 1 << mu
    p = model_plan(wm.flat(mu, l))
    assert [len(r) for r in p["levels"]] == [l, N - l]
    assert wm.info(p) == {"levels": 2, "max_level_rows": N - l, "launches": 2}
    assert wm.launches(p) == [(0, 1), (1, 2)]


def test_self_dependent_row_and_bad_sigma_are_refused():
    mu = 10
    c = wm.self_dependent(mu, 777)
    with pytest.raises(ValueError, match=r"1 of 1024 rows depend on their own output; the first is row 777$"):
        model_plan(c)
    sigma = wm.flat(mu)["sigma"].copy()
    sigma[5] = sigma[6]
    with pytest.raises(ValueError, match="not a permutation"):
        wm.plan(sigma, 1 << mu, [True] * (1 << mu))
    # a two-row cycle, and a row downstream of it: all three have no level
    N, l = 1 << mu, 4
    ia = lambda x: {100: 101, 101: 100, 102: 101}.get(x, x % l)
    c["sigma"] = wm.sigma_of(N, wm._users(N, l, ia, lambda x: (x + 1) % l))
    with pytest.raises(ValueError, match=r"3 of 1024 rows depend on their own output; the first is row 100$"):
        model_plan(c)


def test_wide_edge_cases_in_the_model():
    ok = {"bad_rows": 0, "first_bad_row": None, "bad_copies": 0, "first_bad_copy": None}
    for kw, want in (({}, ok), ({"broken_assert": True}, dict(ok, bad_rows=1, first_bad_row=4)), ({"unequal": True}, dict(ok, bad_copies=1, first_bad_copy=21))):
        c = wm.wide_edge(**kw)
        p = model_plan(c)
        assert p["level"] == [0, 0, 1, 2, None, 3, None, None]
        a, b, cc = wm.generate(c, p, c["public_inputs"], c["free"])
        assert (a[2], b[2], cc[2]) == (6, 15, 7) and (a[3], b[3], cc[3]) == (7, 9, 7 ** 5 + 5)
        assert (a[4], b[4], cc[4]) == (cc[3], cc[3], 77) and a[5] == cc[3] and a[6] == 123 and b[6] == cc[6] == 0
        assert wm.check(c, p, a, b, cc, c["public_inputs"]) == want, kw


def test_mu12_plans_have_a_wide_level_and_a_multi_level_run():
    """what test_gpu_witness.py relies on at mu = 12, for the seed it uses"""
    for kind in KINDS:
        p = model_plan(sample(kind, 12, MU12_SEED))
        assert has_both_paths(p), kind


MU12_SEED = 3


def has_both_paths(p: dict) -> bool:
    sizes = [len(r) for r in p["levels"]]
    return any(n > 256 for n in sizes) and any(e - v >= 2 for v, e in wm.launches(p))


def test_plonk_check_times_the_sampler_row_loop_only_on_request():
    """--sample-only prints the digest line alone, as before; --time-sample R adds one line, the median time of the sampler's row loop"""
    import re
    import subprocess

    tool = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host", "bin", "plonk_check")
    plain = subprocess.run([tool, "--mu", "6", "--gate", "wide", "--sample-only"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and plain.stderr == "" and re.fullmatch(r"circuit sha256 [0-9a-f]{64}\n", plain.stdout)
    timed = subprocess.run([tool, "--mu", "6", "--gate", "wide", "--sample-only", "--time-sample", "2"], capture_output=True, text=True, timeout=120)
    assert timed.returncode == 0 and timed.stderr == ""
    assert re.fullmatch(re.escape(plain.stdout) + r"sample row loop seconds [0-9]+\.[0-9]{6}\n", timed.stdout)
    assert subprocess.run([tool, "--mu", "6", "--time-sample", "2"], capture_output=True, text=True, timeout=120).returncode == 2  # only with that mode
