"""
Witness generation and the witness check on the device: zk_plonk_witness limb for limb against the model of the rules (witness_model.py)
on the four samplers' circuits and on hand-built ones (a chain of ~1000 levels in one workgroup, one wide level, the wide gate's edge
cases), zk_witness_plan_info against the model's plan, the error reports with their exact counts and smallest indices,
zk_plonk_witness_check on the samplers' breaks, prove(witness(...)) end to end, and the compiled host (plonk_check --witness).
"""
import os
import re
import subprocess

import numpy as np
import pytest

import witness_model as wm
from test_witness import KINDS, MU12_SEED, free_of, has_both_paths, model_plan, sample

pytestmark = pytest.mark.gpu

OK = {"bad_rows": 0, "first_bad_row": None, "bad_copies": 0, "first_bad_copy": None}


def light_key(ctx, c: dict) -> dict:
    """what plonk.witness / check_witness read of a proving key: mu, l, the gate kind and the selectors on the device (no SRS, no commitments)"""
    from zkhip import plonk

    gate = plonk.gate_of(c)
    return {"mu": c["mu"], "l": c["l"], "tables": {k: ctx.to_device(np.ascontiguousarray(c[k], dtype=np.uint64)) for k in gate.selectors}, **gate.tag()}


def device_witness(ctx, c: dict, free=None):
    from zkhip import plonk

    pk, plan = light_key(ctx, c), plonk.witness_plan(ctx, c)
    N = 1 << c["mu"]
    f = None if free is None else wm.limbs(free)
    a, b, cc = plonk.witness(ctx, pk, plan, c["public_inputs"], f)
    return pk, plan, [x.download((N, 4)) for x in (a, b, cc)]


def assert_equals_model(ctx, c: dict, free=None, p=None):
    p = p or model_plan(c)
    pk, plan, got = device_witness(ctx, c, free)
    assert plan.info() == wm.info(p)
    want = wm.generate(c, p, c["public_inputs"], free)
    for name, g, w in zip("abc", got, want):
        assert (g == wm.limbs(w)).all(), name
    return pk, plan, got


# mu = 2 for the basic and the wide sampler only: the lookup samplers start at mu = 3
@pytest.mark.parametrize("kind,mu", [(k, mu) for k in KINDS for mu in (2, 3, 5, 12) if mu > 2 or not k.endswith("lookup")])
def test_sampled_circuits_match_the_model(ctx, kind, mu):
    from zkhip import plonk

    c = sample(kind, mu, MU12_SEED if mu == 12 else 7)
    p = model_plan(c)
    if mu == 12:  # one plan with a level above 256 rows AND a multi-level single-workgroup run
        assert has_both_paths(p)
    pk, plan, got = assert_equals_model(ctx, c, free_of(c), p)
    for name, g in zip("abc", got):  # and so the sampler's wires
        assert (g == c[name]).all(), name
    assert plonk.check_witness(ctx, pk, plan, *got, c["public_inputs"]) == OK


def test_chain_of_a_thousand_levels_in_one_workgroup(ctx):
    mu, l = 10, 4
    c = wm.chain(mu, l)
    _, plan, _ = assert_equals_model(ctx, c)
    assert plan.info() == {"levels": (1 << mu) - l + 1, "max_level_rows": l, "launches": 1}


def test_flat_circuit_is_one_wide_level(ctx):
    mu, l = 10, 4
    c = wm.flat(mu, l)
    _, plan, _ = assert_equals_model(ctx, c)
    assert plan.info() == {"levels": 2, "max_level_rows": (1 << mu) - l, "launches": 2}


def test_plans_that_are_refused(ctx):
    mu = 10
    N = 1 << mu
    with pytest.raises(ValueError, match=r"1 of 1024 rows depend on their own output; the first is row 777$"):
        ctx.witness_plan(wm.self_dependent(mu, 777)["sigma"], N)
    ia = lambda x: {100: 101, 101: 100, 102: 101}.get(x, x % 4)
    with pytest.raises(ValueError, match=r"3 of 1024 rows depend on their own output; the first is row 100$"):
        ctx.witness_plan(wm.sigma_of(N, wm._users(N, 4, ia, lambda x: (x + 1) % 4)), N)
    sigma = wm.flat(mu)["sigma"].copy()
    sigma[5] = sigma[6]
    with pytest.raises(ValueError, match="not a permutation"):
        ctx.witness_plan(sigma, N)
    sigma[5] = 3 * N
    with pytest.raises(ValueError, match="not a permutation"):
        ctx.witness_plan(sigma, N)
    for bad_n in (1, 12):
        with pytest.raises(ValueError, match="power of two"):
            ctx.witness_plan(np.arange(3 * bad_n, dtype=np.uint64), bad_n)
    # an output selector that is zero mod r with non-zero limbs (r as it stands) would be a computing row with a zero denominator
    qo = wm.limbs([1] * N)
    qo[9] = np.frombuffer(wm.R.to_bytes(32, "little"), dtype="<u8")
    with pytest.raises(ValueError, match="output selector of row 9 is not reduced below r"):
        ctx.witness_plan(wm.flat(mu)["sigma"], N, ctx.to_device(qo))
    # the gate kind must be the plan's
    from zkhip import plonk

    c = wm.flat(4)
    plan = ctx.witness_plan(c["sigma"], 16)
    plan.wide = True  # (past the Python check)
    with pytest.raises(ValueError, match="wide gate needs a plan built with its output selector"):
        plonk.witness(ctx, dict(light_key(ctx, wm.wide_edge()), mu=4, l=4), plan, c["public_inputs"])


@pytest.mark.parametrize("kw,want,message", [({}, OK, None),
                                             ({"broken_assert": True}, dict(OK, bad_rows=1, first_bad_row=4), r"1 of 8 rows do not satisfy the gate; the first is row 4$"),
                                             ({"unequal": True}, dict(OK, bad_copies=1, first_bad_copy=21), r"1 of 24 slots differ from the value of their class; the first is slot 21$")])
def test_wide_gate_edge_cases(ctx, kw, want, message):
    """qO = 0 assertion rows (satisfied, broken), a qO outside {0, 1}, a class with two computing c slots (equal, unequal), free classes"""
    from zkhip import plonk

    c = wm.wide_edge(**kw)
    p = model_plan(c)
    pk, plan = light_key(ctx, c), plonk.witness_plan(ctx, c)
    assert plan.info() == wm.info(p)
    N = 8
    out = tuple(ctx.alloc(32 * N) for _ in range(3))
    free = ctx.to_device(wm.limbs(c["free"]))
    if message is None:
        ctx.plonk_witness(plan, [pk["tables"][k] for k in wm.WIDE], c["public_inputs"], free, out)
    else:
        with pytest.raises(ValueError, match=message):
            ctx.plonk_witness(plan, [pk["tables"][k] for k in wm.WIDE], c["public_inputs"], free, out)
    # the generated wires are the model's either way, and the check alone gives the same report
    want_w = wm.generate(c, p, c["public_inputs"], c["free"])
    for name, g, w in zip("abc", out, want_w):
        assert (g.download((N, 4)) == wm.limbs(w)).all(), name
    assert wm.check(c, p, *want_w, c["public_inputs"]) == want
    assert plonk.check_witness(ctx, pk, plan, *out, c["public_inputs"]) == want


def test_free_absent_is_free_zero_and_unreduced_free_is_reduced(ctx):
    c = sample("wide-lookup", 5, 7)
    N = 1 << c["mu"]
    _, _, none = device_witness(ctx, c, None)
    _, _, zero = device_witness(ctx, c, [0] * (3 * N))
    for g, z in zip(none, zero):
        assert (g == z).all()
    # free values at or above r (Montgomery limbs as they stand): stored fully reduced
    from zkhip import plonk

    free = free_of(c)
    raw = wm.limbs(free)
    ints = [int.from_bytes(raw[i].astype("<u8").tobytes(), "little") for i in range(3 * N)]
    lifted = [v + wm.R if v + wm.R < 1 << 256 else v for v in ints]
    up = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in lifted), dtype="<u8").astype(np.uint64).reshape(-1, 4)
    pk, plan = light_key(ctx, c), plonk.witness_plan(ctx, c)
    a, b, cc = plonk.witness(ctx, pk, plan, c["public_inputs"], up)
    for name, g in zip("abc", (a, b, cc)):
        assert (g.download((N, 4)) == c[name]).all(), name


@pytest.mark.parametrize("kind", ["basic", "wide"])
def test_check_witness_on_the_samplers_breaks(ctx, kind):
    from zkhip import plonk

    mu = 5
    K = (1 << mu) - 1  # the last row: nothing copies its c
    good = sample(kind, mu, 3)
    pk, plan = light_key(ctx, good), plonk.witness_plan(ctx, good)
    pi = good["public_inputs"]
    assert plonk.check_witness(ctx, pk, plan, good["a"], good["b"], good["c"], pi) == OK
    c = sample(kind, mu, 3, break_gate=K)
    assert plonk.check_witness(ctx, pk, plan, c["a"], c["b"], c["c"], pi) == dict(OK, bad_rows=1, first_bad_row=K)
    c = sample(kind, mu, 3, break_wire=K)
    assert plonk.check_witness(ctx, pk, plan, c["a"], c["b"], c["c"], pi) == dict(OK, bad_copies=1, first_bad_copy=K)
    # a break in the middle spreads to the copies of that c: the device counts what the model counts
    c = sample(kind, mu, 3, break_gate=9)
    p = model_plan(good)
    want = wm.check(good, p, wm.ints(c["a"]), wm.ints(c["b"]), wm.ints(c["c"]), pi)
    assert want["bad_rows"] == 1 and want["first_bad_row"] == 9
    assert plonk.check_witness(ctx, pk, plan, c["a"], c["b"], c["c"], pi) == want
    # wrong public inputs: the input rows fail
    bad_pi = np.array(pi, copy=True)
    bad_pi[1, 0] ^= np.uint64(1)
    assert plonk.check_witness(ctx, pk, plan, good["a"], good["b"], good["c"], bad_pi) == dict(OK, bad_rows=1, first_bad_row=1)


@pytest.mark.parametrize("kind", ["basic", "wide-lookup"])
def test_prove_on_the_generated_witness(ctx, kind):
    """prove(witness(...)) verifies, with the digest of prove on the sampler's wires"""
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk

    mu = 5
    c = sample(kind, mu, 7)
    pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
    pk, vk = plonk.preprocess(ctx, pcs, c, pr.powers_of_g2(wm.ints(c["s"])))
    pi = c["public_inputs"]
    idx = plonk.FIND if "lookup" in c else None
    plan = plonk.witness_plan(ctx, c)
    free = free_of(c)
    a, b, cc = plonk.witness(ctx, pk, plan, pi, None if free is None else wm.limbs(free))
    proof = plonk.prove(ctx, pk, a, b, cc, pi, idx=idx)
    assert plonk.verify(ctx, vk, pi, proof) is True
    assert plonk.proof_digest(proof) == plonk.proof_digest(plonk.prove(ctx, pk, c["a"], c["b"], c["c"], pi, idx=idx))


# ---- the compiled host ----
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scalable-collaborative-zksnark_amd", "host")
PLONK_CHECK = os.path.join(HOST, "bin", "plonk_check")


def _plonk_check(*args):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/plonk_check"])
    r = subprocess.run([PLONK_CHECK, *args], capture_output=True, text=True, timeout=600)
    m = re.search(r"proof sha256 ([0-9a-f]{64})", r.stdout)
    return r, m.group(1) if m else None


@pytest.mark.parametrize("flags", [(), ("--gate", "wide"), ("--lookup", "--find"), ("--gate", "wide", "--lookup", "--find")])
def test_plonk_check_with_a_generated_witness_prints_the_same_digest(flags):
    mu, seed = 8, 7
    r0, plain = _plonk_check("--mu", str(mu), "--seed", str(seed), *flags)
    r1, gen = _plonk_check("--mu", str(mu), "--seed", str(seed), *flags, "--witness")
    assert r0.returncode == 0 and plain, (r0.returncode, r0.stdout, r0.stderr)
    assert r1.returncode == 0 and gen == plain and "witness" in r1.stdout, (r1.returncode, r1.stdout, r1.stderr)
