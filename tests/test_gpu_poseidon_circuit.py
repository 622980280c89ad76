"""
"I know a leaf and a path to this public root" end to end on the device: the tree by zk_poseidon_merkle, the circuit by
poseidon.merkle_circuit, then witness_plan -> witness -> preprocess -> prove -> proof bytes -> verify_bytes through the plonk module as it
stands, at depth 1 (2^9 rows) and depth 2 (2^10 rows); the broken paths are refused by `witness` through its existing messages; the plan is
deeper than the sampled wide circuit's of the same size.
"""
import numpy as np
import pytest

import poseidon_model as pm

pytestmark = pytest.mark.gpu
R = pm.R
SEED = 7


def limbs(xs) -> np.ndarray:
    return np.frombuffer(b"".join(((x << 256) % R).to_bytes(32, "little") for x in xs), dtype="<u8").astype(np.uint64).reshape(-1, 4)


@pytest.fixture(scope="module", params=[1, 2])
def case(request, ctx):
    """per depth, once: the device tree, the path of leaf SEED mod n, the circuit, its plan and keys"""
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk
    from zkhip import poseidon as ps
    from zkhip.field import splitmix_fr

    depth = request.param
    n, index = 1 << depth, SEED % (1 << depth)
    pos = ps.Poseidon(ctx)
    leaves = splitmix_fr(n, SEED)
    tree = pm._ints(pos.merkle(ctx.to_device(leaves), n).download((2 * n - 1, 4)))
    pos.free()
    assert tree == pm.merkle(pm._ints(leaves))
    sibs, bits = ps.merkle_path(tree, n, index)
    circuit, layout, v = ps.merkle_circuit(depth)
    s = splitmix_fr(circuit["mu"] + 1, SEED + 1)
    pcs = dp.PolynomialCommitmentCub.new(ctx, s).mature()
    pk, vk = plonk.preprocess(ctx, pcs, circuit, pr.powers_of_g2(pm._ints(s)))
    return {"depth": depth, "tree": tree, "leaf": tree[index], "sibs": sibs, "bits": bits, "circuit": circuit, "layout": layout, "v": v, "pk": pk, "vk": vk,
            "plan": plonk.witness_plan(ctx, circuit)}


def test_honest_path_is_generated_proved_and_verified(ctx, case):
    from zkhip import plonk
    from zkhip import poseidon as ps

    c, layout, N = case, case["layout"], case["layout"].N
    assert c["circuit"]["mu"] == 8 + c["depth"]
    root = c["tree"][-1]
    pi = limbs([root])
    free = ps.merkle_witness_inputs(layout, c["v"], c["leaf"], c["sibs"], c["bits"])
    a, b, cc = plonk.witness(ctx, c["pk"], c["plan"], pi, free)
    assert plonk.check_witness(ctx, c["pk"], c["plan"], a, b, cc, pi) == {"bad_rows": 0, "first_bad_row": None, "bad_copies": 0, "first_bad_copy": None}
    wires = cc.download((N, 4))
    assert pm._ints(wires[layout.row(c["v"]["out"])][None])[0] == root
    want = pm.evaluate(c["circuit"], [root], {int(s): x for s, x in zip(np.flatnonzero(free.any(axis=1)), pm._ints(free[free.any(axis=1)]))})
    assert (wires == limbs(want["c"])).all()
    proof = plonk.prove(ctx, c["pk"], a, b, cc, pi)
    assert plonk.verify(ctx, c["vk"], pi, proof) is True
    data = plonk.proof_to_bytes(proof)
    assert plonk.verify_bytes(ctx, c["vk"], pi, data) is True
    other = limbs([(root + 1) % R])
    assert plonk.verify(ctx, c["vk"], other, proof) is False and plonk.verify_bytes(ctx, c["vk"], other, data) is False


def test_broken_paths_are_refused_by_witness(ctx, case):
    from zkhip import plonk
    from zkhip import poseidon as ps

    c, layout, N = case, case["layout"], case["layout"].N
    pi = limbs([c["tree"][-1]])
    out_slot = 2 * N + layout.row(c["v"]["out"])
    copy = rf"^zk_plonk_witness: 1 of {3 * N} slots differ from the value of their class; the first is slot {out_slot}$"
    flipped = ps.merkle_witness_inputs(layout, c["v"], c["leaf"], c["sibs"], [c["bits"][0] ^ 1] + c["bits"][1:])
    with pytest.raises(ValueError, match=copy):
        plonk.witness(ctx, c["pk"], c["plan"], pi, flipped)
    wrong = ps.merkle_witness_inputs(layout, c["v"], c["leaf"], [(c["sibs"][0] + 1) % R] + c["sibs"][1:], c["bits"])
    with pytest.raises(ValueError, match=copy):
        plonk.witness(ctx, c["pk"], c["plan"], pi, wrong)
    two = ps.merkle_witness_inputs(layout, c["v"], c["leaf"], c["sibs"], [2] + c["bits"][1:])
    with pytest.raises(ValueError, match=rf"^zk_plonk_witness: 1 of {N} rows do not satisfy the gate; the first is row 1; 1 of {3 * N} slots differ"):
        plonk.witness(ctx, c["pk"], c["plan"], pi, two)


def test_the_plan_is_deep_and_narrow(ctx, case):
    from zkhip import plonk

    mu = case["circuit"]["mu"]
    info = case["plan"].info()
    sampled = plonk.witness_plan(ctx, plonk.sample_circuit_wide(mu, SEED)).info()
    # three levels per round (S-box, two linear rows) and five before each hash
    assert info["levels"] > 190 * case["depth"] and info["levels"] > sampled["levels"]
    assert info["max_level_rows"] < sampled["max_level_rows"]
