"""
Proof bytes end to end on the device (zkhip.proof_io): prove at mu = 4 for the basic and the wide gate, with and without the lookup
sample, encode, verify_bytes; the device and the host path give one record; an order-3 point added to one point of every part of the
record, one flipped byte per part and a header of the other gate kind are all refused.  What plonk.verify itself says on an off-subgroup
point is not asserted: include/zkhip.h calls that value meaningless.
"""
import numpy as np
import pytest

import g1check_model as gm
import zerocheck_model as zm

pytestmark = pytest.mark.gpu

MU = 4
T3 = (0, 2)  # a point of order 3
_PROVED = {}


def _proved(ctx, kind, lookup):
    """(vk, public inputs, record, bytes), proved once per kind"""
    if (kind, lookup) not in _PROVED:
        from zkhip import dist_primitive as dp
        from zkhip import pairing as pr
        from zkhip import plonk

        if lookup:
            c = plonk.sample_circuit_lookup(MU, 31, gate=kind)
        else:
            c = (plonk.sample_circuit_wide if kind else plonk.sample_circuit)(MU, 31)
        pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
        pk, vk = plonk.preprocess(ctx, pcs, c, pr.powers_of_g2(zm.ints(c["s"])))
        proof = plonk.prove(ctx, pk, c["a"], c["b"], c["c"], c["public_inputs"], **({"idx": c["idx"]} if lookup else {}))
        _PROVED[(kind, lookup)] = (vk, c["public_inputs"], proof, plonk.proof_to_bytes(proof))
    return _PROVED[(kind, lookup)]


def _point_offsets(kind, lookup):
    from zkhip import proof_io

    offs, spans, pos = [], [], 26
    for name, what, shape in proof_io._layout(kind, lookup, MU):
        n = proof_io._count(shape)
        size = (48 if what == "g1" else 32) * n
        if what == "g1":
            offs += [pos + 48 * i for i in range(n)]
        spans.append((name, pos, size))
        pos += size
    return offs, spans


KINDS = [(None, False), (None, True), ("wide", False), ("wide", True)]


@pytest.mark.parametrize("kind,lookup", KINDS)
def test_bytes_verify_and_both_paths_give_the_prover_s_record(ctx, kind, lookup):
    from zkhip import plonk, proof_io

    vk, pi, proof, data = _proved(ctx, kind, lookup)
    assert len(data) == proof_io.proof_size(kind, lookup, MU)
    assert plonk.verify_bytes(ctx, vk, pi, data) is True
    dev, host = plonk.proof_from_bytes(ctx, data), plonk.proof_from_bytes(None, data, host=True)
    assert plonk.proof_digest(dev) == plonk.proof_digest(host) == plonk.proof_digest(proof)
    assert plonk.proof_to_bytes(dev) == data
    assert plonk.check_points(ctx, proof) == [] and plonk.check_points(ctx, dev) == []
    assert plonk.verify(ctx, vk, pi, dev) is True


@pytest.mark.parametrize("kind,lookup", KINDS)
def test_an_order_3_point_added_to_one_point_of_every_part_is_refused_and_named(ctx, kind, lookup):
    from zkhip import plonk, proof_io

    vk, pi, proof, data = _proved(ctx, kind, lookup)
    parts = proof_io.point_parts(kind, lookup, MU)
    offs, _ = _point_offsets(kind, lookup)
    names = ["commitments", "v_commitment", "batch.opening", "v_batch.opening"] + (["lookup.commitments", "lookup.batch.opening"] if lookup else [])
    assert sorted(set(p for p, _ in parts)) == sorted(names)
    for j, name in enumerate(names):
        slots = [s for s, (p, _) in enumerate(parts) if p == name]
        slot = slots[j % len(slots)]
        part, idx = parts[slot]
        P = gm.decompress_check(bytes(data[offs[slot]:offs[slot] + 48]))[1]
        bad_point = gm.add(P, T3)
        assert gm.on_curve(bad_point) and not gm.in_g1(bad_point)
        bad = bytearray(data)
        bad[offs[slot]:offs[slot] + 48] = gm.compress(bad_point)
        assert plonk.verify_bytes(ctx, vk, pi, bytes(bad)) is False, name
        with pytest.raises(ValueError) as err:
            plonk.proof_from_bytes(ctx, bytes(bad))
        assert str(err.value) == proof_io.describe(part, idx, 3), name
        # the same point in a record that is already a dict
        rec = plonk.proof_from_bytes(ctx, data)
        arr = proof_io._get(rec, name)
        arr.reshape(-1, 18)[idx] = gm.words(bad_point)
        assert plonk.check_points(ctx, rec) == [(part, idx, 3)], name


@pytest.mark.parametrize("kind,lookup", KINDS)
def test_one_flipped_byte_per_part_and_the_other_header_are_refused(ctx, kind, lookup):
    from zkhip import plonk

    vk, pi, _, data = _proved(ctx, kind, lookup)
    _, spans = _point_offsets(kind, lookup)
    rng = np.random.default_rng(3)
    for name, pos, size in [("header", 0, 26)] + spans:
        at = pos + int(rng.integers(size))
        bad = bytearray(data)
        bad[at] ^= 1 << int(rng.integers(8))
        assert plonk.verify_bytes(ctx, vk, pi, bytes(bad)) is False, (name, at)
    other = bytearray(data)
    other[8] ^= 1  # the other gate kind: the body no longer has the header's length
    assert plonk.verify_bytes(ctx, vk, pi, bytes(other)) is False
    with pytest.raises(ValueError):
        plonk.parse_proof(bytes(other))
    # a well-formed proof of the other kind against this vk: the header disagrees with the vk
    o_vk, o_pi, _, o_data = _proved(ctx, "wide" if kind is None else None, lookup)
    assert plonk.verify_bytes(ctx, vk, pi, o_data) is False and plonk.verify_bytes(ctx, o_vk, o_pi, o_data) is True
    assert plonk.verify_bytes(ctx, vk, pi, data) is True
