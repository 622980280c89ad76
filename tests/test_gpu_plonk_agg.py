"""
plonk.verify_many / verify_agg / proof_io.verify_bytes_many against the existing verifier: the aggregated verdicts equal
[plonk.verify(...) for ...] on three proofs per case -- basic gate, wide gate, basic gate with a lookup, at mu = 3 and 4.
The basic and the wide case hold three DIFFERENT proofs under one key (the wires of three sets of public inputs, plonk.witness); the
lookup case repeats one proof, as its rows must hit the table.
"""
import numpy as np
import pytest

import zerocheck_model as zm

pytestmark = pytest.mark.gpu

KINDS = ["basic", "wide", "lookup"]


@pytest.fixture(scope="module")
def cases(ctx):
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk
    from zkhip.field import splitmix_fr

    made = {}

    def get(mu, kind):
        if (mu, kind) in made:
            return made[mu, kind]
        sample = {"basic": plonk.sample_circuit, "wide": plonk.sample_circuit_wide, "lookup": plonk.sample_circuit_lookup}[kind]
        c = sample(mu, 7)
        pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
        pk, vk = plonk.preprocess(ctx, pcs, c, pr.powers_of_g2(zm.ints(c["s"])))
        pi = c["public_inputs"]
        items = [(pi, plonk.prove(ctx, pk, c["a"], c["b"], c["c"], pi, idx=c.get("idx")))]
        if kind == "lookup":
            items += [items[0], items[0]]
        else:
            plan = plonk.witness_plan(ctx, c)
            for seed in (1, 2):
                pi2 = splitmix_fr(c["l"], 9000 + seed)
                a, b, cc = plonk.witness(ctx, pk, plan, pi2)
                items.append((pi2, plonk.prove(ctx, pk, a, b, cc, pi2)))
            assert len({plonk.proof_digest(p) for _, p in items}) == 3
        made[mu, kind] = (vk, items)
        return made[mu, kind]

    return get


def _flipped_opening(proof):
    """the field checks hold, the pairing does not: a moved point of the first instance's opening"""
    opening = np.array(proof["batch"]["opening"], copy=True)
    opening[0] = opening[-1]
    return dict(proof, batch=dict(proof["batch"], opening=opening))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mu", [3, 4])
def test_verify_many_equals_verify(ctx, cases, mu, kind):
    from zkhip import ZkError, plonk, proof_io
    from zkhip import dist_primitive as dp
    from zkhip.field import Q_MOD, int_to_limbs, limbs_to_int

    vk, items = cases(mu, kind)
    each = lambda its: [plonk.verify(ctx, vk, pi, p) for pi, p in its]
    # all honest
    assert each(items) == [True] * 3 and plonk.verify_many(ctx, vk, items) == [True] * 3
    # one proof with a flipped opening point: exactly that proof is False
    for j in (2,):  # (the first proof's: verify_agg below)
        bad = list(items)
        bad[j] = (items[j][0], _flipped_opening(items[j][1]))
        assert plonk.field_checks(vk, *bad[j]) is True
        want = [k != j for k in range(3)]
        assert each(bad) == want and plonk.verify_many(ctx, vk, bad) == want, j
    # one proof failing failed_checks (another proof's public inputs / a flipped round): it never reaches the aggregate
    broken = dict(items[1][1], g_values=np.array(items[1][1]["g_values"], copy=True))
    broken["g_values"].reshape(-1)[0] ^= np.uint64(1)
    bad = [items[0], (items[1][0], broken), items[2]]
    assert plonk.failed_checks(vk, *bad[1]) != []
    assert plonk.verify_many(ctx, vk, bad) == each(bad) == [True, False, True]
    assert plonk.agg_openings(vk, bad)[0] == [0, 2] and len(plonk.agg_openings(vk, bad)[1]) == 2 * (3 if kind == "lookup" else 2)
    # one proof with an opening point off the curve (y + 1), one with a coordinate that is not canonical (x + q): the field checks hold, the
    # aggregate REFUSES the point (a status, ZK_ERR_INVALID), and the one-by-one pass names the proof
    for how in ("off the curve", "not canonical"):
        opening = np.array(items[2][1]["batch"]["opening"], copy=True).reshape(-1, 18)
        if how == "off the curve":
            opening[1, 6] ^= np.uint64(1)
        else:
            opening[1, :6] = int_to_limbs(limbs_to_int(opening[1, :6]) + Q_MOD, 6)
        off = [items[0], items[1], (items[2][0], dict(items[2][1], batch=dict(items[2][1]["batch"], opening=opening)))]
        assert plonk.field_checks(vk, *off[2]) is True
        alive, openings = plonk.agg_openings(vk, off)
        assert alive == [0, 1, 2]
        with pytest.raises(ZkError, match="proof point 1 of opening %d: %s" % (2 * len(openings) // 3, "the point is not on the curve" if how == "off the curve"
                                                                                 else "a coordinate is not canonical")):
            dp.verify_agg(ctx, vk["pcs"][1], openings)
        with pytest.raises(ZkError):  # (plonk.verify leaves such a record to proof_io.check_points: it raises the library's refusal)
            plonk.verify(ctx, vk, *off[2])
        assert plonk.verify_many(ctx, vk, off) == [True, True, False], how
    # an empty list, a list of broken records only
    assert plonk.verify_many(ctx, vk, []) == []
    assert plonk.verify_many(ctx, vk, [bad[1], (items[0][0], {})]) == [False, False]
    # verify_agg equals verify
    assert plonk.verify_agg(ctx, vk, *items[0]) is True
    assert plonk.verify_agg(ctx, vk, items[0][0], _flipped_opening(items[0][1])) is False
    assert plonk.verify_agg(ctx, vk, *bad[1]) is False
    # the encodings
    datas = [(pi, proof_io.proof_to_bytes(p)) for pi, p in items]
    assert proof_io.verify_bytes_many(ctx, vk, datas) == [True] * 3
    assert proof_io.verify_bytes(ctx, vk, *datas[0], aggregate=True) is True and proof_io.verify_bytes(ctx, vk, *datas[0]) is True
    mixed = [datas[0], (datas[1][0], datas[1][1][:-1]), (datas[2][0], proof_io.proof_to_bytes(_flipped_opening(items[2][1])))]
    assert proof_io.verify_bytes_many(ctx, vk, mixed) == [proof_io.verify_bytes(ctx, vk, pi, d) for pi, d in mixed] == [True, False, False]
    assert proof_io.verify_bytes_many(ctx, vk, []) == []
