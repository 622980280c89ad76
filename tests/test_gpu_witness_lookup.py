"""
Witness generation through lookups on the device: zk_plonk_witness_lookup limb for limb against the model of the rules
(witness_lookup_model.py) on sample_circuit_lookup_fn and on hand-built circuits (a chain of ~1000 lookup levels in one workgroup, one flat
level), zk_witness_plan_info against the model's plan, the key table under the knob find_force_slot, the refusals with their exact
numbers, zk_plonk_witness_check_lookup, prove(..., idx=FIND) on the generated wires, and the compiled host (plonk_check --lookup-fn).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import witness_lookup_model as wlm
import witness_model as wm
from test_witness_lookup import OK, SEEDS, a_break_row, sampled

pytestmark = pytest.mark.gpu

LK = ("qk", "t0", "t1", "t2")


class _Knob:
    """sets a tuning knob of the library for a with-block and puts back what it found (in a finally: __exit__ runs on every way out)"""

    def __init__(self, key, value):
        from zkhip._lib import test_hooks

        self.lib, self.key, self.value = test_hooks(), key, value

    def __enter__(self):
        v = ctypes.c_long(0)
        assert self.lib.zk_dbg_tune_get(self.key, ctypes.byref(v)) == 0
        self.found = v.value
        assert self.lib.zk_dbg_tune(self.key, self.value) == 0

    def __exit__(self, *exc):
        self.lib.zk_dbg_tune(self.key, self.found)


def light_key(ctx, c: dict) -> dict:
    from zkhip import plonk

    return plonk.witness_key(ctx, c)


def device_witness(ctx, c: dict, free):
    """-> (pk, plan, the three wire columns as arrays, the error message or None): the wires are downloaded whether or not the witness
    was refused"""
    from zkhip import plonk

    pk, plan = light_key(ctx, c), plonk.witness_plan(ctx, c, lookup=True)
    N = 1 << c["mu"]
    out = tuple(ctx.alloc(32 * N) for _ in range(3))
    sels, pi, lk = plonk._witness_args(pk, plan, c["public_inputs"])
    message = None
    try:
        ctx.plonk_witness(plan, sels, pi, None if free is None else ctx.to_device(wm.limbs(free)), out, **lk)
    except ValueError as e:
        message = str(e)
    return pk, plan, [x.download((N, 4)) for x in out], message


def assert_equals_model(ctx, c: dict, free, p=None):
    p = p or wlm.plan(c)
    pk, plan, got, message = device_witness(ctx, c, free)
    assert message is None, message
    assert plan.info() == wlm.info(p)
    want = wlm.generate(c, p, c["public_inputs"], free)
    for name, g, w in zip("abc", got, want):
        assert (g == wm.limbs(w)).all(), name
    return pk, plan, got


@pytest.mark.parametrize("mu", [3, 5, 9, 12])
def test_sampled_circuits_match_the_model(ctx, mu):
    from zkhip import plonk

    c, p, free = sampled(mu, SEEDS[0])
    if mu >= 9:  # a level above 256 rows (the grid) AND a multi-level single-workgroup run
        assert any(len(r) > 256 for r in p["levels"]) and any(e - v >= 2 for v, e in wlm.launches(p))
    pk, plan, got = assert_equals_model(ctx, c, free, p)
    for name, g in zip("abc", got):  # and so the sampler's wires
        assert (g == c[name]).all(), name
    assert plonk.check_witness(ctx, pk, plan, *got, c["public_inputs"]) == OK
    # the property of the rules: zk_lookup3_find on the generated wires gives the y the generator used
    idx, _ = ctx.lookup3_find([ctx.to_device(g) for g in got], [pk["tables"][k] for k in LK[1:]], pk["tables"]["qk"], 1 << mu)
    assert (idx.download((1 << mu,), dtype=np.uint32) == c["idx"]).all()


def test_chain_of_a_thousand_lookup_levels_in_one_workgroup(ctx):
    mu, l = 10, 4
    c = wlm.chain(mu, l)
    _, plan, _ = assert_equals_model(ctx, c, c["free"])
    assert plan.info() == {"levels": (1 << mu) - l, "max_level_rows": l + 1, "launches": 1}


def test_flat_circuit_is_one_grid_launch(ctx):
    mu = 10
    c = wlm.flat(mu)
    _, plan, _ = assert_equals_model(ctx, c, c["free"])
    assert plan.info() == {"levels": 1, "max_level_rows": 1 << mu, "launches": 1}


def _broken_table(c: dict, entry: int, delta: int) -> dict:
    t2 = wm.ints(c["lookup"]["t2"])
    t2[entry] += delta
    return dict(c, lookup=dict(c["lookup"], t2=wm.limbs(t2)))


@pytest.mark.parametrize("mu", [3, 6])
def test_find_force_slot_changes_nothing(ctx, mu):
    """one collision chain from slot 0, and one that wraps round the end of the 2N slots: the wires, the reports and the refusals are those
    of the hash"""
    from zkhip import plonk

    N = 1 << mu
    c, p, free = sampled(mu, SEEDS[0]) if mu == 3 else (lambda c: (c, wlm.plan(c), c["free"]))(wlm.flat(mu, 4, 2))  # 16 entries, padded to 64
    K = a_break_row(c) if mu == 3 else N - 1
    broken_free = list(free)
    broken_free[K] += 1 << 4  # the a of lookup row K leaves the table
    bad_table = _broken_table(c, N - 2, 1)

    def run():
        _, _, wires, message = device_witness(ctx, c, free)
        _, plan, broken, refusal = device_witness(ctx, c, broken_free)
        report = plonk.check_witness(ctx, light_key(ctx, c), plan, *broken, c["public_inputs"])
        with pytest.raises(ValueError) as e:
            plonk.witness_plan(ctx, bad_table, lookup=True)
        return [w.tobytes() for w in wires], message, [w.tobytes() for w in broken], refusal, report, str(e.value)

    plain = run()
    assert plain[1] is None and plain[4]["bad_lookups"] == 1 and plain[4]["first_bad_lookup"] == K
    assert plain[3].endswith(f"1 of {N} rows with qk = 1 hold a triple that is no table entry; the first is row {K}")
    for start in (0, 2 * N - 1):
        with _Knob(b"find_force_slot", start):
            assert run() == plain, start
    # a plan keeps the start slot it was built with: the knob may change between its creation and its use
    with _Knob(b"find_force_slot", 0):
        pk, plan = light_key(ctx, c), plonk.witness_plan(ctx, c, lookup=True)
    a, b, cc = plonk.witness(ctx, pk, plan, c["public_inputs"], wm.limbs(free))
    assert [x.download((N, 4)).tobytes() for x in (a, b, cc)] == plain[0]


def test_refusals_with_exact_numbers(ctx):
    from zkhip import plonk

    c = wlm.flat(3, 2, 1)  # N = 8: the table has 4 entries and is padded with entry 3
    with pytest.raises(ValueError, match=r"1 of 8 table entries repeat the pair \(t0, t1\) of an earlier entry with another t2; the first is entry 6$"):
        plonk.witness_plan(ctx, _broken_table(c, 6, 1), lookup=True)
    with pytest.raises(ValueError, match=r"4 of 8 table entries repeat the pair .* the first is entry 4$"):
        plonk.witness_plan(ctx, _broken_table(c, 3, 1), lookup=True)  # the FIRST entry of the pair changed: the four later ones differ
    plonk.witness_plan(ctx, c, lookup=True)  # the same pair repeated with the same t2: accepted
    qk = wm.ints(c["lookup"]["qk"])
    with pytest.raises(ValueError, match=r"1 of 8 entries of qk are neither 0 nor 1; the first is row 5$"):
        plonk.witness_plan(ctx, dict(c, lookup=dict(c["lookup"], qk=wm.limbs(qk[:5] + [2] + qk[6:]))), lookup=True)
    with pytest.raises(ValueError, match=r"2 of 64 rows depend on their own output; the first is row 33$"):
        plonk.witness_plan(ctx, wlm.self_dependent(), lookup=True)
    with pytest.raises(ValueError, match="needs a circuit with a lookup"):
        plonk.witness_plan(ctx, {k: v for k, v in c.items() if k != "lookup"}, lookup=True)
    # a lookup call on a plain plan, and a plain call on a lookup plan
    pk = light_key(ctx, c)
    sels, lk = [pk["tables"][k] for k in wm.WIDE], {"qk": pk["tables"]["qk"], "ts": [pk["tables"][k] for k in LK[1:]]}
    plain, with_lk = plonk.witness_plan(ctx, c), plonk.witness_plan(ctx, c, lookup=True)
    w = tuple(ctx.alloc(32 * 8) for _ in range(3))
    for call in (lambda: ctx.plonk_witness(plain, sels, c["public_inputs"], None, w, **lk), lambda: ctx.plonk_witness_check(plain, sels, c["public_inputs"], *w, **lk)):
        with pytest.raises(ValueError, match="the plan was built without a lookup"):
            call()
    for call in (lambda: ctx.plonk_witness(with_lk, sels, c["public_inputs"], None, w), lambda: ctx.plonk_witness_check(with_lk, sels, c["public_inputs"], *w)):
        with pytest.raises(ValueError, match="the plan was built with a lookup"):
            call()


def test_break_row_is_refused_with_the_models_numbers(ctx):
    from zkhip import plonk

    mu, seed = 5, SEEDS[1]
    good, p, _ = sampled(mu, seed)
    K = a_break_row(good)
    c = plonk.sample_circuit_lookup_fn(mu, seed, break_row=K)
    free = wm.ints(c["free"])
    want_w = wlm.generate(c, p, c["public_inputs"], free)
    want = wlm.check(c, p, *want_w, c["public_inputs"])
    assert want == dict(OK, bad_lookups=1, first_bad_lookup=K)
    pk, plan, got, message = device_witness(ctx, c, free)
    assert message.endswith(f"zk_plonk_witness_lookup: 1 of {1 << mu} rows with qk = 1 hold a triple that is no table entry; the first is row {K}")
    for name, g, w in zip("abc", got, want_w):  # the wires hold what was generated: c = 0 on the miss
        assert (g == wm.limbs(w)).all(), name
    assert plonk.check_witness(ctx, pk, plan, *got, c["public_inputs"]) == want


def test_check_witness_counts_bad_lookups(ctx):
    from zkhip import plonk

    # the c of one lookup-computing row replaced by another value of the table's range: a bad lookup there, and bad copies where it is copied
    mu = 5
    c, p, _ = sampled(mu, SEEDS[0])
    N = 1 << mu
    a, b, cc = (wm.ints(c[k]) for k in "abc")
    users = [x for x in range(N) if p["kind"][x] == wlm.LOOKUP and any(src == (False, x) for s, src in enumerate(p["src"]) if s != 2 * N + x)]
    K = users[0]
    cc[K] ^= 1
    want = wlm.check(c, p, a, b, cc, c["public_inputs"])
    assert want["bad_lookups"] == 1 and want["first_bad_lookup"] == K and want["bad_copies"] >= 1 and want["bad_rows"] == 0
    pk, plan = light_key(ctx, c), plonk.witness_plan(ctx, c, lookup=True)
    assert plonk.check_witness(ctx, pk, plan, c["a"], c["b"], wm.limbs(cc), c["public_inputs"]) == want
    # the multiplication-table sampler: its qk = 1 rows are gate-computing, and the table only checks them
    good = plonk.sample_circuit_lookup(mu, 7, gate="wide")
    K = int(np.flatnonzero(good["lookup"]["qk"][:, 0])[-1])
    c = plonk.sample_circuit_lookup(mu, 7, gate="wide", break_lookup=K)
    pk, plan = light_key(ctx, c), plonk.witness_plan(ctx, c, lookup=True)
    assert plan.info() == wm.info(wlm.plan(c))
    assert plonk.check_witness(ctx, pk, plan, c["a"], c["b"], c["c"], c["public_inputs"]) == dict(OK, bad_lookups=1, first_bad_lookup=K)
    assert plonk.check_witness(ctx, pk, plan, good["a"], good["b"], good["c"], good["public_inputs"]) == OK


@pytest.mark.parametrize("mu", [5, 9])
def test_prove_with_find_on_the_generated_witness(ctx, mu):
    """prove(witness(...), idx=FIND) verifies, with the digest of prove on the sampler's wires and the sampler's idx"""
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk

    c, _, _ = sampled(mu, SEEDS[0])
    pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
    pk, vk = plonk.preprocess(ctx, pcs, c, pr.powers_of_g2(wm.ints(c["s"])))
    pi = c["public_inputs"]
    plan = plonk.witness_plan(ctx, c, lookup=True)
    a, b, cc = plonk.witness(ctx, pk, plan, pi, c["free"])
    proof = plonk.prove(ctx, pk, a, b, cc, pi, idx=plonk.FIND)
    assert plonk.verify(ctx, vk, pi, proof) is True
    assert plonk.proof_digest(proof) == plonk.proof_digest(plonk.prove(ctx, pk, c["a"], c["b"], c["c"], pi, idx=c["idx"]))


# ---- the compiled host ----
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scalable-collaborative-zksnark_amd", "host")
PLONK_CHECK = os.path.join(HOST, "bin", "plonk_check")


def _plonk_check(*args):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/plonk_check"])
    r = subprocess.run([PLONK_CHECK, *args], capture_output=True, text=True, timeout=600)
    m = re.search(r"proof sha256 ([0-9a-f]{64})", r.stdout)
    return r, m.group(1) if m else None


@pytest.mark.parametrize("mu", [5, 9])
def test_plonk_check_lookup_fn_prints_one_digest_in_both_hosts(ctx, mu):
    """the sampler's wires and indices, the generated wires with the device's own search, and the Python host: one digest"""
    from zkhip import dist_primitive as dp
    from zkhip import plonk

    seed = SEEDS[0]
    flags = ("--mu", str(mu), "--seed", str(seed), "--gate", "wide", "--lookup-fn")
    r0, plain = _plonk_check(*flags)
    r1, gen = _plonk_check(*flags, "--witness", "--find")
    assert r0.returncode == 0 and plain, (r0.returncode, r0.stdout, r0.stderr)
    assert r1.returncode == 0 and gen == plain and "witness" in r1.stdout, (r1.returncode, r1.stdout, r1.stderr)
    c, _, _ = sampled(mu, seed)
    pk, _ = plonk.preprocess(ctx, dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature(), c)
    assert plonk.proof_digest(plonk.prove(ctx, pk, c["a"], c["b"], c["c"], c["public_inputs"], idx=c["idx"])) == plain


def test_plonk_check_lookup_fn_refuses_a_broken_row():
    c, _, _ = sampled(5, SEEDS[1])
    K = a_break_row(c)
    flags = ("--mu", "5", "--seed", str(SEEDS[1]), "--gate", "wide", "--lookup-fn", "--break-lookup", str(K))
    r, digest = _plonk_check(*flags, "--witness", "--find")
    assert r.returncode == 3 and digest is None, (r.returncode, r.stdout, r.stderr)
    assert f"1 of 32 rows with qk = 1 hold a triple that is no table entry; the first is row {K}" in r.stderr
    r, digest = _plonk_check(*flags)  # the sampler's broken wires and indices: zk_lookup3_multiplicities refuses (it counts, and names no row)
    assert r.returncode == 3 and digest is None and "1 of 32 rows are not in the table" in r.stderr, (r.returncode, r.stdout, r.stderr)
