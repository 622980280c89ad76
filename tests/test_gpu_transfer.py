"""
The transfer circuit on the device (zkhip.poseidon.merkle_transfer_circuit at (depth, bits) = (1, 8) and (2, 16)): the caller gives
balances, amount and paths, the witness generator makes every inverse and bit; witness -> preprocess -> prove -> bytes -> verify_bytes
accepts, a flipped bit of the proof bytes is rejected, and amount 0, an amount above the balance, an overflowing receiver and a wrong
sibling are refused by `witness` with the numbers the model of the rules (advice_model.py) gives.
"""
import numpy as np
import pytest

import advice_model as am
import transfer_cases as tc
import witness_model as wm

pytestmark = pytest.mark.gpu

CASES = [(1, 8), (2, 16)]


@pytest.fixture(scope="module", params=CASES, ids=lambda p: f"depth{p[0]}-bits{p[1]}")
def setup(ctx, request):
    from zkhip import plonk

    case = tc.case(*request.param)
    return case, plonk.witness_key(ctx, case["circuit"]), plonk.witness_plan(ctx, case["circuit"])


def test_the_plan_is_the_models(setup):
    case, _, plan = setup
    p = case.setdefault("plan", am.plan(case["circuit"]))
    assert plan.info() == am.info(p) and am.ADVICE in p["kind"]


def test_a_good_transfer_is_proved_and_verified(ctx, setup):
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk
    from zkhip.field import splitmix_fr

    case, _, plan = setup
    circuit = case["circuit"]
    pi, free = tc.inputs(case, "good")
    s = splitmix_fr(circuit["mu"] + 1, 8)
    pcs = dp.PolynomialCommitmentCub.new(ctx, s).mature()
    pk, vk = plonk.preprocess(ctx, pcs, circuit, pr.powers_of_g2(wm.ints(s)))
    a, b, c = plonk.witness(ctx, pk, plan, pi, free)
    N = 1 << circuit["mu"]
    p = case.setdefault("plan", am.plan(circuit))
    want = am.generate(circuit, p, pi, wm.ints(free))
    for name, g, w in zip("abc", (a, b, c), want):
        assert (g.download((N, 4)) == wm.limbs(w)).all(), name
    raw = plonk.proof_to_bytes(plonk.prove(ctx, pk, a, b, c, pi))
    assert plonk.verify_bytes(ctx, vk, pi, raw)
    flipped = bytearray(raw)
    flipped[len(raw) // 2] ^= 0x10
    assert plonk.verify_bytes(ctx, vk, pi, bytes(flipped)) is False


@pytest.mark.parametrize("name", ["zero", "over", "overflow", "sibling"])
def test_a_bad_transfer_is_refused_as_the_model_predicts(ctx, setup, name):
    from zkhip import plonk

    case, key, plan = setup
    rep = tc.model_report(case, name)
    assert (rep["bad_rows"] > 0, rep["bad_copies"] > 0) == tc.EXPECTED[name]
    pi, free = tc.inputs(case, name)
    with pytest.raises(ValueError) as e:
        plonk.witness(ctx, key, plan, pi, free)
    assert str(e.value) == tc.message(rep, 1 << case["circuit"]["mu"])
