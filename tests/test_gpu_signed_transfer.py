"""
The Schnorr circuit on the device (zkhip.jubjub.schnorr_circuit, mu = 14): the wires `witness` generates equal the model's limb for limb,
witness -> preprocess -> prove -> bytes -> verify_bytes accepts, the same proof under another key's public inputs is rejected, and a forged
signature (s + 1 mod l) and a wrong message are refused by `witness` with the model's count and first index.  Then
merkle_signed_transfer_circuit(depth = 2, bits = 8) on a 4-leaf tree built with Poseidon.merkle / update: accepted when signed by the sender;
refused by `witness` when signed by the receiver's key and when the amount differs from the signed one.  One prove per circuit.
"""
import pytest

import advice_model as am
import jubjub_model as jm
import signed_transfer_cases as sc
import transfer_cases as tc
import witness_model as wm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(ctx):
    from zkhip import jubjub as jj
    from zkhip import plonk

    circuit, layout, v = jj.schnorr_circuit()
    return circuit, layout, v, am.plan(circuit), plonk.witness_key(ctx, circuit), plonk.witness_plan(ctx, circuit)


def inputs(setup, PK, m, sig):
    from zkhip import jubjub as jj

    return wm.limbs([PK[0], PK[1], m % jm.R, 0]), jj.schnorr_inputs(setup[1], setup[2], sig)


def test_the_plan_is_the_models(setup):
    assert setup[5].info() == am.info(setup[3])


def test_a_signature_is_proved_and_verified(ctx, setup):
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk
    from zkhip.field import splitmix_fr

    circuit, layout, v, p, _, plan = setup
    _, PK, m, sig = jm.signed_cases()[0]
    pi, free = inputs(setup, PK, m, sig)
    s = splitmix_fr(circuit["mu"] + 1, 8)
    pcs = dp.PolynomialCommitmentCub.new(ctx, s).mature()
    pk, vk = plonk.preprocess(ctx, pcs, circuit, pr.powers_of_g2(wm.ints(s)))
    a, b, c = plonk.witness(ctx, pk, plan, pi, free)
    N = 1 << circuit["mu"]
    want = am.generate(circuit, p, pi, wm.ints(free))
    for name, g, w in zip("abc", (a, b, c), want):
        assert (g.download((N, 4)) == wm.limbs(w)).all(), name
    raw = plonk.proof_to_bytes(plonk.prove(ctx, pk, a, b, c, pi))
    assert plonk.verify_bytes(ctx, vk, pi, raw)
    _, PK2, _, _ = jm.signed_cases()[1]
    assert plonk.verify_bytes(ctx, vk, wm.limbs([PK2[0], PK2[1], m % jm.R, 0]), raw) is False


@pytest.mark.parametrize("name", ["forged_s", "wrong_message"])
def test_a_bad_signature_is_refused_as_the_model_predicts(ctx, setup, name):
    from zkhip import plonk

    circuit, layout, v, p, key, plan = setup
    _, PK, m, (Rp, s) = jm.signed_cases()[0]
    pi, free = inputs(setup, PK, m, (Rp, (s + 1) % jm.L)) if name == "forged_s" else inputs(setup, PK, m ^ 1, (Rp, s))
    rep = am.check(circuit, p, *am.generate(circuit, p, pi, wm.ints(free)), pi)
    assert rep["bad_rows"] + rep["bad_copies"] > 0
    with pytest.raises(ValueError) as e:
        plonk.witness(ctx, key, plan, pi, free)
    assert str(e.value) == tc.message(rep, 1 << circuit["mu"])


# ---- the signed transfer ----
@pytest.fixture(scope="module")
def signed(ctx):
    from zkhip import jubjub as jj
    from zkhip import plonk

    circuit, layout, v = jj.merkle_signed_transfer_circuit(sc.DEPTH, sc.BITS)
    return circuit, layout, v, am.plan(circuit), plonk.witness_key(ctx, circuit), plonk.witness_plan(ctx, circuit)


def test_the_device_trees_are_the_cases(ctx):
    """the three trees of the case -- before, after the sender's write, after the receiver's -- built with Poseidon.merkle and two updates"""
    from zkhip import poseidon as ps

    c = sc.case("good")
    pos = ps.Poseidon(ctx)
    try:
        tree = pos.merkle(ctx.to_device(wm.limbs(c["trees"][0][:sc.N])), sc.N)
        assert (tree.download((2 * sc.N - 1, 4)) == wm.limbs(c["trees"][0])).all()
        for idx, want in ((sc.SENDER, c["trees"][1]), (sc.RECEIVER, c["trees"][2])):
            pos.update(tree, sc.N, [idx], wm.limbs([want[idx]]))
            assert (tree.download((2 * sc.N - 1, 4)) == wm.limbs(want)).all()
    finally:
        pos.free()


def test_a_signed_transfer_is_proved_and_verified(ctx, signed):
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk
    from zkhip.field import splitmix_fr

    circuit, layout, v, p, _, plan = signed
    c = sc.case("good")
    pi, free = wm.limbs(c["pi"]), sc.free_of(layout, v, c)
    s = splitmix_fr(circuit["mu"] + 1, 8)
    pcs = dp.PolynomialCommitmentCub.new(ctx, s).mature()
    pk, vk = plonk.preprocess(ctx, pcs, circuit, pr.powers_of_g2(wm.ints(s)))
    a, b, cc = plonk.witness(ctx, pk, plan, pi, free)
    N = 1 << circuit["mu"]
    want = am.generate(circuit, p, pi, wm.ints(free))
    for name, g, w in zip("abc", (a, b, cc), want):
        assert (g.download((N, 4)) == wm.limbs(w)).all(), name
    raw = plonk.proof_to_bytes(plonk.prove(ctx, pk, a, b, cc, pi))
    assert plonk.verify_bytes(ctx, vk, pi, raw)
    assert plonk.verify_bytes(ctx, vk, wm.limbs([c["pi"][0], sc.case("other_amount")["pi"][1]]), raw) is False


@pytest.mark.parametrize("name", ["receiver_signed", "other_amount"])
def test_a_transfer_the_sender_did_not_sign_is_refused(ctx, signed, name):
    from zkhip import plonk

    circuit, layout, v, p, key, plan = signed
    c = sc.case(name)
    pi, free = wm.limbs(c["pi"]), sc.free_of(layout, v, c)
    rep = am.check(circuit, p, *am.generate(circuit, p, pi, wm.ints(free)), pi)
    assert rep["bad_rows"] + rep["bad_copies"] > 0
    with pytest.raises(ValueError) as e:
        plonk.witness(ctx, key, plan, pi, free)
    assert str(e.value) == tc.message(rep, 1 << circuit["mu"])
